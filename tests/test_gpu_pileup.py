"""GPU: allele counts per template position from the consensus reads (mipgen_accel_reads_consensus_pileup, `mipgen_count -pileup`).  Every
comparison is exact equality of the whole counts array and of the totals against tests/pileup_ref.py - plain loops over groups and positions - in two ways:
the oracle on the groups the device itself fetched, and end to end from the reads through tests/consensus_ref.py.  Probes are cut from a random genome (the
device calls) or from a golden genome on both strands (the command line), so that molecule lengths, read lengths and molecule counts are the test's to choose."""
import faulthandler
import json
import os
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi, synth
from tests import consensus_ref as CR
from tests import helpers as H
from tests import pileup_ref as PR
from tests import reads_ref as R
from tests.test_gpu_reads import BASES, TABLES, _accel, random_tag
from tests.test_gpu_samples import GOLDEN_PLAIN, clean_reads_uneven_depth_inputs, draw_barcodes, plain_session_digest
from tests.test_pileup_cpu import clean_window, synthetic_row
from tests.test_reads_cpu import HEADER

pytestmark = pytest.mark.gpu
COUNT_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_count")
E_INVALID, E_NOMEM, E_STATE = -1, -5, -6
WG = 256                                      # PILEUP_WG_CELL (reads_common.h): above it a cell takes a workgroup per round
ARM = 16
TAGS = (8, 0)                                 # 65,536 tags: enough distinct ones for 5,000 molecules in a cell
SETTINGS = ((1, 0), (1, 3), (1, 40), (2, 0))  # (min_family, min_quality)


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


def test_the_threshold_is_the_kernels():
    text = open(os.path.join(os.path.dirname(capi.LIB_PATH), "csrc", "reads_common.h")).read()
    assert f"#define PILEUP_WG_CELL {WG} " in text


# ---- probes and molecules -------------------------------------------------------------------------------------------------------------------------------
def cut_probes(genome, lengths):
    """One probe per entry of `lengths`: its molecule M is that many bases of the genome, its arms the first and the last ARM bases of M."""
    mols = [genome[700 * k + 300:700 * k + 300 + n] for k, n in enumerate(lengths)]
    assert all(set(m) <= set(b"ACGT") and len(m) >= 2 * ARM for m in mols)
    return mols, [(m[:ARM], m[-ARM:]) for m in mols]


def tag_of(k, n=8):
    return bytes(b"ACGT"[(k >> (2 * (n - 1 - j))) & 3] for j in range(n))


class Lane:
    """The read pairs of a test, molecule by molecule; every molecule gets a tag of its own."""

    def __init__(self, rng):
        self.rng, self.ext, self.lig, self.eq, self.lq, self.idx, self.n_tags = rng, [], [], [], [], [], 0

    def molecule(self, M, n_e, n_l, family=1, subs=(), ext_subs=(), err=0.0, qual=None, index=b"", member_edit=None):
        """`family` pairs of one molecule of M: extension reads of n_e bases behind the tag, ligation reads of n_l (beyond M: random backbone).  subs: (t, base)
        the molecule truly carries; ext_subs: seen in its extension reads only; err: sequencing errors per base behind the arms (substitutions and N);
        qual: a quality byte for every base (default: random 35..74); member_edit(m, e, l, eq, lq) -> the four of member m, edited."""
        rng = self.rng
        Mv = bytearray(M)
        for t, b in subs:
            Mv[t] = b
        Me = bytearray(Mv)
        for t, b in ext_subs:
            Me[t] = b
        tag = tag_of(self.n_tags); self.n_tags += 1
        for m in range(family):
            e = bytearray((bytes(Me) + random_tag(rng, max(n_e - len(M), 0)))[:n_e])
            l = bytearray((R.revcomp(bytes(Mv)) + random_tag(rng, max(n_l - len(M), 0)))[:n_l])
            for s in (e, l):
                for j in np.flatnonzero(rng.random(len(s)) < err):
                    if j >= ARM:
                        s[j] = ord("N") if rng.random() < 0.2 else BASES[rng.integers(0, 4)]
            e, l = tag + bytes(e), bytes(l)
            q = (lambda n: bytes([qual]) * n) if qual is not None else (lambda n: rng.integers(35, 75, n).astype(np.uint8).tobytes())
            eq, lq = q(len(e)), q(len(l))
            if member_edit:
                e, l, eq, lq = member_edit(m, e, l, eq, lq)
            self.ext.append(e); self.lig.append(l); self.eq.append(eq); self.lq.append(lq); self.idx.append(index)

    def shuffled(self):
        order = self.rng.permutation(len(self.ext))
        return [[col[i] for i in order] for col in (self.ext, self.lig, self.eq, self.lq, self.idx)]


def compare(acc, got_groups, want_groups, mol_len, rows=(0,), settings=SETTINGS):
    """The device against the oracle on the device's own groups and on the groups of consensus_ref, for every row and setting; returns {(row, setting): result}."""
    assert got_groups == want_groups
    n = len(mol_len)
    out = {}
    for row in rows:
        for mf, mq in settings:
            counts, totals = acc.consensus_pileup(mol_len, row, mf, mq)
            w_counts, w_totals = PR.pileup(want_groups, mol_len, n, row, mf, mq)
            assert counts.dtype == np.int32 and counts.shape == (sum(mol_len), 5)
            assert np.array_equal(counts, w_counts), (row, mf, mq, np.flatnonzero((counts != w_counts).any(axis=1))[:5])
            assert totals == w_totals, (row, mf, mq)
            assert totals["bases"] == int(counts[:, :4].sum()) and totals["discordant"] == int(counts[:, 4].sum())
            out[(row, (mf, mq))] = (counts, totals)
    return out


def session(acc, arms, lane_cols, barcodes=None, chunks=1):
    ext, lig, eq, lq, idx = lane_cols
    got = acc.consensus_reads(arms, ext, lig, eq, lq, idx if barcodes else None, barcodes, 0, TAGS, chunks=chunks)
    want = CR.consensus_reads(arms, ext, lig, eq, lq, idx if barcodes else None, barcodes, 0, TAGS)
    return got[4], want[4]


# ---- template lengths, side lengths, overlap --------------------------------------------------------------------------------------------------------------
def test_template_lengths_side_lengths_and_overlap(acc, genome):
    """Molecules of 63, 64, 65, 129 and 200 bases - every remainder of a round of 64 positions - and one probe of length 1 among them; on each, consensus reads
    shorter than, as long as and longer than the molecule on either side, a gap between the sides, an overlap of exactly one, full overlap and the bare arms;
    1 to 8 molecules per cell (every remainder of the unrolled loop), sequencing errors, families of 1 to 3."""
    rng = np.random.default_rng(401)
    lengths = [63, 64, 80, 65, 129, 200]
    mols, arms = cut_probes(genome, lengths)
    mol_len = [63, 64, 1, 65, 129, 200]                           # probe 2: a molecule length of 1 (its reads run through from position 1 on)
    L = Lane(rng)
    shapes = lambda n: [(n, n), (n + 7, n - 11), (n - 9, n + 5), (n + 4, n + 3), (n // 2 - 3, n // 2 - 3), (20, n - 20 + 1), (n - 16, 17), (ARM, ARM)]
    for p, M in enumerate(mols):
        for k, (n_e, n_l) in enumerate(shapes(len(M))[:p + 3]):
            subs = [(int(rng.integers(ARM, len(M) - ARM)), BASES[rng.integers(0, 4)])] if k % 2 else []
            L.molecule(M, n_e, n_l, family=1 + k % 3, subs=subs, err=0.03)
    got, want = session(acc, arms, L.shuffled())
    per_cell = sorted(sum(1 for g in got if g[0] == p) for p in range(len(mols)))
    assert per_cell == [3, 4, 5, 6, 7, 8]
    for p, n in enumerate(mol_len):                               # every side length relative to the molecule is there
        sides = [(len(g[3]), len(g[5])) for g in got if g[0] == p]
        assert any(e > n for e, _ in sides) and any(l > n for _, l in sides)
        if n > 1:
            assert any(e == n for e, _ in sides) and any(e < n for e, _ in sides) and any(l == n for _, l in sides) and any(l < n for _, l in sides)
    res = compare(acc, got, want, mol_len)
    counts, totals = res[(0, (1, 0))]
    assert totals["groups"] == totals["used"] == 33 and totals["discordant"] > 0
    at = np.cumsum([0] + mol_len)
    assert counts[at[2]:at[3]].sum() == 5                         # the probe of length 1: one position, five molecules, each counted once somewhere
    assert (counts[at[5]:at[6]].sum(axis=1) == 0).sum() == 0 and counts[at[5] + 100].sum() >= 5
    # the same reads against other molecule lengths (the device never sees the molecule, only its length): lengths that cut every read short, and one beyond them
    for other in ([1, 1, 1, 1, 1, 1], [64, 63, 65, 129, 200, 63], [300, 128, 192, 1, 2, 127]):
        compare(acc, got, want, other, settings=((1, 0), (2, 3)))


# ---- molecules per cell ------------------------------------------------------------------------------------------------------------------------------------
def test_molecules_per_cell(acc, genome):
    """Cells of 1 to 8 molecules, of threshold - 1, threshold and threshold + 1, + 5, + 9, + 13 (one wavefront; a workgroup whose wavefronts take 64 to 68
    molecules each, so that their unrolled loops end in every remainder), and of 5,000; an empty probe between two populated ones, the first and the last
    probe populated."""
    rng = np.random.default_rng(409)
    sizes = [5000, 1, 2, 0, 3, 4, 5, 6, 7, 8, WG - 1, WG, WG + 1, WG + 5, WG + 9, WG + 13, 0, 9]
    lengths = [40 if s == 5000 else 65 if s > 8 else 129 for s in sizes]                                  # (the large cell on a short molecule: the oracles' time)
    mols, arms = cut_probes(genome, lengths)
    L = Lane(rng)
    for p, (M, s) in enumerate(zip(mols, sizes)):
        for k in range(s):
            subs = [(int(rng.integers(0, len(M))), BASES[rng.integers(0, 4)])] if k % 5 == 0 else []
            ext_subs = [(int(rng.integers(ARM, len(M))), BASES[rng.integers(0, 4)])] if k % 7 == 0 else []
            subs = [s_ for s_ in subs if ARM <= s_[0] < len(M) - ARM]                                       # (the arms stay exact: every pair is assigned)
            ext_subs = [s_ for s_ in ext_subs if s_[0] < len(M) - ARM]
            L.molecule(M, len(M) - 3 * (k % 4), len(M) - 2 * (k % 3), family=2 if k % 11 == 0 else 1, subs=subs, ext_subs=ext_subs, qual=ord("#") + (k % 3) * 19)
    got, want = session(acc, arms, L.shuffled(), chunks=3)
    assert [sum(1 for g in got if g[0] == p) for p in range(len(sizes))] == sizes
    res = compare(acc, got, want, lengths, settings=((1, 0), (2, 3)))
    counts, totals = res[(0, (1, 0))]
    assert totals["groups"] == sum(sizes) and totals["discordant"] > 0
    at = np.cumsum([0] + lengths)
    assert counts[at[0] + 30, :4].sum() + counts[at[0] + 30, 4] == 5000                                   # every molecule of the large cell votes at a position both sides cover
    assert not counts[at[3]:at[4]].any() and not counts[at[-3]:at[-2]].any()                              # the empty probes
    assert counts[at[-2]:].any() and counts[:at[1]].any()


# ---- content -----------------------------------------------------------------------------------------------------------------------------------------------
def test_planted_content(acc, genome):
    """Substitutions seen by the extension side only, by the ligation side only and by both; a disagreement of the two sides; N in a consensus from a tied vote;
    '#' and 'I' positions under min_quality 0, 3 and 40; min_family 1, 2 and one above every family."""
    rng = np.random.default_rng(419)
    mols, arms = cut_probes(genome, [100, 100, 100])
    M = mols[1]
    other = lambda t: b"ACGT"[(b"ACGT".index(M[t]) + 1) & 3]
    col = lambda b: b"ACGT".index(b)
    L = Lane(rng)
    I = ord("I")
    L.molecule(M, 60, 60, qual=I)                                                                           # m0: clean.  Extension: t 0..59, ligation: t 99..40
    L.molecule(M, 60, 60, qual=I, subs=[(30, other(30)), (80, other(80)), (50, other(50))])                # m1: a variant molecule
    L.molecule(M, 60, 60, qual=I, ext_subs=[(45, other(45))])                                              # m2: the sides disagree at t 45

    def tie(m, e, l, eq, lq):                                                                               # m3: two members, A against C at t 20, equal qualities
        return (e[:8 + 20] + (b"A" if m == 0 else b"C") + e[8 + 21:], l, eq, lq)

    L.molecule(M, 60, 60, family=2, qual=I, member_edit=tie)

    def low(m, e, l, eq, lq):                                                                               # m4: quality 2 at t 10 and at j 5 (t 94)
        return (e, l, eq[:8 + 10] + b"#" + eq[8 + 11:], lq[:5] + b"#" + lq[6:])

    L.molecule(M, 60, 60, qual=I, member_edit=low)
    L.molecule(mols[0], 100, 100, qual=I); L.molecule(mols[2], 100, 100, family=2, qual=I)
    got, want = session(acc, arms, L.shuffled())
    m3 = [g for g in got if g[0] == 1 and g[2] == 2][0]
    assert m3[3][20:21] == b"N" and m3[4][20:21] == b"#" and m3[4][19:20] == b"I"
    res = compare(acc, got, want, [100, 100, 100], settings=((1, 0), (1, 3), (1, 40), (2, 0), (3, 0)))
    c0, t0 = res[(0, (1, 0))]
    c0 = c0[100:200]

    def expect(t, ref, alt=0, disc=0):
        r = [0] * 5
        r[col(M[t])] += ref
        if alt:
            r[col(other(t))] += alt
        r[4] = disc
        return r

    assert c0[5].tolist() == expect(5, 5) and c0[70].tolist() == expect(70, 5) and c0[55].tolist() == expect(55, 5)       # one side, the other, both (once)
    assert c0[30].tolist() == expect(30, 4, 1) and c0[80].tolist() == expect(80, 4, 1) and c0[50].tolist() == expect(50, 4, 1)
    assert c0[45].tolist() == expect(45, 4, 0, 1) and c0[20].tolist() == expect(20, 4)
    assert t0 == {"groups": 7, "used": 7, "bases": 7 * 100 - 2, "discordant": 1}                            # (the row: five molecules here, one on each other probe)
    for mq in (3, 40):                                                                                      # '#' is 2: dropped from 3 on; 'I' is 40: kept at 40
        c, t = res[(0, (1, mq))]
        c = c[100:200]
        assert c[10].tolist() == expect(10, 4) and c[94].tolist() == expect(94, 4) and c[11].tolist() == expect(11, 5) and c[20].tolist() == expect(20, 4)
        assert t == {"groups": 7, "used": 7, "bases": 7 * 100 - 4, "discordant": 1}
    c, t = res[(0, (2, 0))]
    assert c[100:200].sum(axis=1).tolist() == [1] * 20 + [0] + [1] * 79 and t["used"] == 2 and t["groups"] == 7 and c[:100].sum() == 0 and c[200:].sum() == 100
    c, t = res[(0, (3, 0))]
    assert not c.any() and t == {"groups": 7, "used": 0, "bases": 0, "discordant": 0}


# ---- rows and chunks -----------------------------------------------------------------------------------------------------------------------------------------
def rows_lane(genome, rng):
    mols, arms = cut_probes(genome, [90, 129, 64, 75])
    barcodes = draw_barcodes(rng, 3, 8)                                                                     # sample 2 gets no pair: a row without groups
    L = Lane(rng)
    for p, M in enumerate(mols):
        for k in range(3 + 2 * p):
            index = barcodes[k % 2] if k % 5 != 4 else random_tag(rng, 8)                                   # every fifth molecule: no sample (undetermined)
            L.molecule(M, 70, 66, family=1 + k % 2, subs=[(ARM + 3 * k, b"ACGT"[k % 4])], err=0.02, index=index)
    # the same tag on the same probe in two samples: two molecules
    L.n_tags = 40000
    L.molecule(mols[0], 70, 66, index=barcodes[0], qual=ord("I"))
    L.n_tags = 40000
    L.molecule(mols[0], 70, 66, index=barcodes[1], qual=ord("I"), subs=[(40, b"ACGT"[(b"ACGT".index(mols[0][40]) + 2) & 3])])
    return mols, arms, barcodes, L


def test_rows(acc, genome):
    rng = np.random.default_rng(421)
    mols, arms, barcodes, L = rows_lane(genome, rng)
    mol_len = [len(m) for m in mols]
    cols = L.shuffled()
    got, want = session(acc, arms, cols, barcodes)
    n = len(arms)
    assert {g[0] // n for g in got} == {0, 1, 3} and len([g for g in got if g[1] == CR.tag_code(tag_of(40000))]) == 2
    res = compare(acc, got, want, mol_len, rows=(2, 0, 1, 3), settings=((1, 0), (2, 3)))                   # row 2 first: the row without groups
    assert not res[(2, (1, 0))][0].any() and res[(2, (1, 0))][1] == {"groups": 0, "used": 0, "bases": 0, "discordant": 0}
    assert sum(res[(r, (1, 0))][1]["groups"] for r in range(4)) == len(got)
    assert not np.array_equal(res[(0, (1, 0))][0], res[(1, (1, 0))][0])
    for r in (2, 0, 1, 0, 0, 3):                                                                            # any order, and the same row twice
        counts, totals = acc.consensus_pileup(mol_len, r)
        assert np.array_equal(counts, res[(r, (1, 0))][0]) and totals == res[(r, (1, 0))][1]
    # without barcodes the same pairs are one row
    got1, want1 = session(acc, arms, cols)
    one = compare(acc, got1, want1, mol_len, settings=((1, 0),))
    assert one[(0, (1, 0))][1]["groups"] == len(got1) == len(got) - 1                                       # (the shared tag is one molecule now)


def test_chunks_do_not_change_the_table(acc, genome):
    rng = np.random.default_rng(431)
    mols, arms, barcodes, L = rows_lane(genome, rng)
    mol_len = [len(m) for m in mols]
    cols = L.shuffled()
    got, want = session(acc, arms, cols, barcodes, chunks=1)
    first = compare(acc, got, want, mol_len, rows=(0, 1, 3), settings=((1, 0),))
    for chunks in (3, 17):
        got_c, _ = session(acc, arms, cols, barcodes, chunks=chunks)
        assert got_c == got
        for r in (0, 1, 3):
            counts, totals = acc.consensus_pileup(mol_len, r)
            assert np.array_equal(counts, first[(r, (1, 0))][0]) and totals == first[(r, (1, 0))][1], (chunks, r)


# ---- state, refusals, the untouched handle ---------------------------------------------------------------------------------------------------------------------
def test_state_refusals_and_untouched_handle(genome):
    g12 = synth.random_genome(12000, 5)
    P = capi.make_params(130, 140, score_method=capi.SCORE_LOGISTIC, arm_pairs=synth.arm_pairs_from_sums([43, 44]))
    a = capi.Accel(P)
    try:
        a.upload([capi.build_region(g12, "1", 5000, 5055, P, bwa_mode="hashed", label="s1")])
        a.score_resident(capi.SCORE_LOGISTIC)
        s0, r0 = a.download()

        def unchanged():
            s, r = a.download()
            assert np.array_equal(s.view(np.int64), s0.view(np.int64)) and np.array_equal(r, r0)

        rng = np.random.default_rng(433)
        mols, arms, barcodes, L = rows_lane(genome, rng)
        mol_len = [len(m) for m in mols]
        n = len(arms)
        ext, lig, eq, lq, idx = L.shuffled()
        lib, h = a.lib, a.h
        i32p = capi.C.POINTER(capi.C.c_int32)
        lens = np.array(mol_len, dtype=np.int32)
        counts = np.full((sum(mol_len), 5), -7, dtype=np.int32)
        tot = capi.PileupTotals()
        pile = lambda lens_=lens, n_=n, row=0, mf=1, mq=0, out=counts: lib.mipgen_accel_reads_consensus_pileup(
            h, lens_.ctypes.data_as(i32p) if lens_ is not None else None, n_, row, mf, mq, out.ctypes.data_as(i32p) if out is not None else None, capi.C.byref(tot))
        # nothing is held: before any session, and while one is open
        assert pile() == E_STATE and b"holds no consensus reads" in lib.mipgen_accel_last_error()
        arr = capi.probe_array(arms)
        assert lib.mipgen_accel_reads_open_consensus(h, arr, n, 8, 0, 0, None, 0, 0, 0) == 0
        assert pile() == E_STATE
        assert lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, None) == 0
        # a handle with zero groups gives zeros
        assert pile() == 0 and not counts.any() and (tot.groups, tot.used, tot.bases, tot.discordant) == (0, 0, 0, 0)
        assert a.last_kernel_ms(11) < 0
        unchanged()
        # results held: every refusal with its code, and nothing written by a refused call
        got = a.consensus_reads(arms, ext, lig, eq, lq, idx, barcodes, 0, TAGS)[4]
        counts[:] = -7
        bad = lens.copy(); bad[2] = 0
        for kw in ({"lens_": None}, {"n_": n - 1}, {"n_": n + 1}, {"lens_": bad}, {"row": -1}, {"row": 4}, {"mf": 0}, {"mf": -3}, {"mq": -1}, {"mq": 41}):
            assert pile(**kw) == E_INVALID, kw
        assert pile(mq=41) == E_INVALID and b"min_quality 41" in lib.mipgen_accel_last_error()
        assert pile(row=4) == E_INVALID and b"row 4" in lib.mipgen_accel_last_error()
        assert (counts == -7).all()
        # the call itself: counts and totals may each be NULL; a fetch before and after is identical; the dense results download unchanged
        sizes = capi.ConsensusSizes(len(got), sum(len(g[3]) for g in got), sum(len(g[5]) for g in got))
        assert a.consensus_fetch(sizes) == got
        assert pile() == 0
        want_counts, want_totals = PR.pileup(got, mol_len, n, 0)
        assert np.array_equal(counts, want_counts) and {f[0]: getattr(tot, f[0]) for f in capi.PileupTotals._fields_} == want_totals
        assert pile(out=None) == 0 and tot.bases == want_totals["bases"]
        assert lib.mipgen_accel_reads_consensus_pileup(h, lens.ctypes.data_as(i32p), n, 3, 1, 0, counts.ctypes.data_as(i32p), None) == 0
        assert np.array_equal(counts, PR.pileup(got, mol_len, n, 3)[0])
        assert a.consensus_fetch(sizes) == got
        unchanged()
        # timing off: nothing booked; on: the kernels of the last call
        assert a.last_kernel_ms(11) < 0
        a.set_timing(True)
        timed, _ = a.consensus_pileup(mol_len, 1)
        assert a.last_kernel_ms(11) > 0 and np.array_equal(timed, PR.pileup(got, mol_len, n, 1)[0])
        a.set_timing(False)
        a.consensus_pileup(mol_len, 1)
        assert a.last_kernel_ms(11) < 0
        # the next open drops the reads
        assert lib.mipgen_accel_reads_open(h, arr, n, 8, 0, 0) == 0
        assert pile() == E_STATE
        assert lib.mipgen_accel_reads_finish(h, None, None, None) == 0
        assert pile() == E_STATE
        unchanged()
    finally:
        a.close()


def test_destroy_with_results_held(genome):
    rng = np.random.default_rng(439)
    mols, arms, barcodes, L = rows_lane(genome, rng)
    ext, lig, eq, lq, idx = L.shuffled()
    a = _accel()
    a.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=TAGS)
    counts, totals = a.consensus_pileup([len(m) for m in mols])                                             # the reads and the pileup's buffers held at destroy
    assert totals["bases"] > 0
    a.close()


@pytest.mark.parametrize("name,key", TABLES[:1])
def test_a_plain_session_afterwards_is_the_recorded_one(acc, genome, name, key):
    rng = np.random.default_rng(443)
    mols, arms, barcodes, L = rows_lane(genome, rng)
    ext, lig, eq, lq, idx = L.shuffled()
    acc.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=TAGS)
    acc.consensus_pileup([len(m) for m in mols])
    t_rows, t_ext, t_lig = clean_reads_uneven_depth_inputs(name, key)
    got = acc.count_reads([(r[6], r[10]) for r in t_rows], t_ext, t_lig, want_assignment=True)
    recorded = json.load(open(GOLDEN_PLAIN))
    assert plain_session_digest(*got) == recorded[f"{name}/{key}"]["sha256"]


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------------------
def write_fastq_q(path, reads, quals):
    with open(path, "wb") as fh:
        for i, (r, q) in enumerate(zip(reads, quals)):
            fh.write(b"@r%d\n" % i + r + b"\n+\n" + q + b"\n")


def _run(argv, cwd):
    return subprocess.run(argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


@pytest.mark.parametrize("with_barcodes", [False, True])
def test_cli_equals_the_oracle(tmp_path, with_barcodes):
    """A small table cut from a golden genome on both strands and FASTQ with planted substitutions: the -pileup file byte for byte and the stderr line, with
    and without -consensus (whose FASTQ files are what they are without -pileup), and with -pileup_min_family 2."""
    g = H.golden_genome()
    rng = np.random.default_rng(449 + with_barcodes)
    t_rows, at = [], 5000
    for k in range(8):
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
        for k in range(2 + 3 * (p % 3)):
            tag = random_tag(rng, 8)
            Mv = bytearray(M)
            if k % 2:
                t = int(rng.integers(24, len(M) - 24))
                Mv[t] = b"ACGT"[(b"ACGT".index(M[t]) + 1 + k % 3) & 3]                                     # a variant molecule
            index = barcodes[int(rng.integers(0, 2))] if rng.random() < 0.85 else random_tag(rng, 8)
            for m in range(1 + (k + p) % 3):
                e = bytearray(tag[:5] + bytes(Mv)[:95] + random_tag(rng, max(95 - len(M), 0)))
                l = bytearray(tag[5:] + R.revcomp(bytes(Mv))[:97] + random_tag(rng, max(97 - len(M), 0)))
                if m == 1:
                    e[40] = ord("N"); l[50] = BASES[rng.integers(0, 4)]                                    # sequencing errors in one member
                ext.append(bytes(e)); lig.append(bytes(l)); idx.append(index)
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
    base = _run(common, str(tmp_path))
    assert base.returncode == 0, base.stderr.decode()
    plain_counts = open(tmp_path / "counts.tsv", "rb").read()
    cons = _run(common + ["-consensus", "smc"], str(tmp_path))
    assert cons.returncode == 0, cons.stderr.decode()
    # -pileup alone
    text, line = PR.pileup_file(want[4], t_rows, lab)
    assert text.count(b"\n") > 500 and b"\t-\t" in text and b"\t+\t" in text and int(line.split()[9]) > 0      # (nonref: the planted variants)
    p = _run(common + ["-pileup", "pile.tsv"], str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert open(tmp_path / "pile.tsv", "rb").read() == text
    assert p.stderr.decode() == base.stderr.decode() + line
    assert open(tmp_path / "counts.tsv", "rb").read() == plain_counts and not os.path.exists(tmp_path / "pile.tsv.ext.fq")
    # with -consensus: the FASTQ files of a run without -pileup, the consensus line, then the pileup line
    both = _run(common + ["-pileup", "pile2.tsv", "-consensus", "smc2"], str(tmp_path))
    assert both.returncode == 0, both.stderr.decode()
    assert open(tmp_path / "pile2.tsv", "rb").read() == text and both.stderr.decode() == cons.stderr.decode() + line
    for side in ("ext", "lig"):
        assert open(tmp_path / f"smc2.{side}.fq", "rb").read() == open(tmp_path / f"smc.{side}.fq", "rb").read() != b""
    # -pileup_min_family 2 and -pileup_min_quality 40
    text2, line2 = PR.pileup_file(want[4], t_rows, lab, 2, 40)
    p = _run(common + ["-pileup", "pile3.tsv", "-pileup_min_family", "2", "-pileup_min_quality", "40"], str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert open(tmp_path / "pile3.tsv", "rb").read() == text2 != text and p.stderr.decode() == base.stderr.decode() + line2
