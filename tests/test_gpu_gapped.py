"""GPU: the pileup with indels (mipgen_accel_reads_consensus_pileup_gapped, `mipgen_count -pileup FILE -pileup_indels W`).  Every comparison is exact
equality of the whole counts array and of the totals against tests/gapped_ref.py - the full table per (molecule, side), a plain traceback, plain loops - in two
ways: the oracle on the groups the device itself fetched, and end to end from the reads through tests/consensus_ref.py."""
import faulthandler
import json
import os

import numpy as np
import pytest

from mipgen_amd import capi, synth
from tests import consensus_ref as CR
from tests import gapped_ref as G
from tests import helpers as H
from tests import pileup_ref as PR
from tests import reads_ref as R
from tests.test_gapped_cpu import plant, substitution_lane
from tests.test_gpu_pileup import ARM, COUNT_BIN, TAGS, WG, Lane, _run, cut_probes, session, write_fastq_q
from tests.test_gpu_reads import TABLES, _accel, random_tag
from tests.test_gpu_samples import GOLDEN_PLAIN, clean_reads_uneven_depth_inputs, draw_barcodes, plain_session_digest
from tests.test_pileup_cpu import clean_window, synthetic_row
from tests.test_reads_cpu import HEADER

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -6
PAD = b"GATTACAGATTACAGATTACAGATTACA"
KEYS = ("groups", "used", "bases", "discordant", "deletions", "insertions", "ins_discordant", "gapped_sides")


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


def variant(L, M, Me, Ml, n_e, n_l, family=1, qual=None, index=b""):
    """`family` pairs of a molecule of probe M whose extension reads show Me and whose ligation reads show revcomp(Ml) (beyond them: backbone)."""
    def edit(m, e, l, eq, lq):
        e2, l2 = e[:TAGS[0]] + (Me + PAD)[:n_e], (G.revcomp(Ml) + PAD)[:n_l]
        q = (lambda n: bytes([qual]) * n) if qual is not None else (lambda n: L.rng.integers(35, 75, n).astype(np.uint8).tobytes())
        return e2, l2, q(len(e2)), q(len(l2))

    assert Me[:ARM] == M[:ARM] and Ml[-ARM:] == M[-ARM:]                           # the arms stay exact: every pair is assigned
    L.molecule(M, n_e, n_l, family=family, qual=qual, index=index, member_edit=edit)


def compare(acc, got_groups, want_groups, mols, rows=(0,), settings=((1, 0),), Ws=(4,)):
    """The device against the oracle on the device's own groups and on the groups of consensus_ref, for every row, setting and W; {(row, setting, W): result}."""
    assert got_groups == want_groups
    n, lens, out = len(mols), [len(m) for m in mols], {}
    for row in rows:
        for mf, mq in settings:
            for W in Ws:
                counts, totals = acc.consensus_pileup_gapped(mols, lens, row, mf, mq, W)
                w_counts, w_totals = G.pileup(want_groups, mols, n, row, mf, mq, W)
                assert counts.dtype == np.int32 and counts.shape == (sum(lens), 8)
                assert np.array_equal(counts, w_counts), (row, mf, mq, W, np.flatnonzero((counts != w_counts).any(axis=1))[:5])
                assert totals == w_totals and tuple(totals) == KEYS, (row, mf, mq, W, totals, w_totals)
                out[(row, (mf, mq), W)] = (counts, totals)
    return out


# ---- template lengths, band widths, every kind of planted indel ---------------------------------------------------------------------------------------------
def test_lengths_bands_and_planted_indels(acc, genome):
    """Molecules of 40, 63, 64, 65, 129 and 200 bases under W = 1, 4 and 15.  On each: deletions of 1, 2, 3, 4, 5, 15 and 16 bases (1, 3, W and W + 1 for every
    W) and insertions of 1, 3, 4 and 15, in both reads; an indel directly behind either arm and within three bases of either read end; one seen by one side only
    because the other read is too short; one planted in one read only; a read-through extension read with a deletion (its end cell lies on column L); N next to
    the indel; families of 1 and 2."""
    rng = np.random.default_rng(463)
    lengths = [40, 63, 64, 65, 129, 200]
    mols, arms = cut_probes(genome, lengths)
    L = Lane(rng)
    for p, M in enumerate(mols):
        n, k = len(M), 0
        mid = n // 2
        for kind, size in (("del", 1), ("del", 2), ("del", 3), ("del", 4), ("del", 5), ("del", 15), ("del", 16), ("ins", 1), ("ins", 3), ("ins", 4), ("ins", 15)):
            if kind == "del" and n - size < 2 * ARM + 2:
                continue
            Mv = plant(M, kind, min(mid, n - ARM - size - 1) if kind == "del" else mid, size, rng)
            variant(L, M, Mv, Mv, len(Mv), len(Mv), family=1 + k % 2); k += 1                                  # both reads see it whole
            variant(L, M, Mv, Mv, len(Mv) + 9, len(Mv) - 5)                                                    # the extension read runs through into the backbone
        for kind in ("del", "ins"):
            variant(L, M, plant(M, kind, ARM, 1, rng), plant(M, kind, n - ARM - (kind == "del"), 1, rng), n, n)   # directly behind each side's arm
            Mv = plant(M, kind, n - ARM - 2, 2, rng)
            variant(L, M, Mv, Mv, len(Mv) - ARM + 1, ARM + 3)                                                  # within three bases of both read ends
            Mv = plant(M, kind, ARM + 2, 1, rng)
            variant(L, M, Mv, Mv, len(Mv), ARM + 1)                                                            # the ligation read is too short to see it
            variant(L, M, Mv, M, n, n)                                                                         # planted in the extension read only
            variant(L, M, M, plant(M, kind, n - ARM - 3, 2, rng), n, n)                                        # in the ligation read only
            Mv = plant(M, kind, ARM + 4, 3, rng)
            at = ARM + 4 - 1
            variant(L, M, Mv[:at] + b"N" + Mv[at + 1:], Mv, len(Mv), len(Mv), qual=ord("I"))                    # N next to the indel
    got, want = session(acc, arms, L.shuffled())
    res = compare(acc, got, want, mols, settings=((1, 0), (2, 20)), Ws=(1, 4, 15))
    for W in (1, 4, 15):
        t = res[(0, (1, 0), W)][1]
        assert t["deletions"] > 0 and t["insertions"] > 0 and t["ins_discordant"] > 0 and t["discordant"] > 0 and t["gapped_sides"] > 100


def test_repeats_in_the_overlap_are_not_discordant(acc, genome):
    """An indel inside a homopolymer and inside a dinucleotide repeat, seen by both reads: both sides place it at the same position, so `discordant` and
    `ins_discordant` stay 0."""
    rng = np.random.default_rng(467)
    base, _ = cut_probes(genome, [60, 60])
    mols = [base[0][:28] + b"AAAAAAAA" + base[0][36:], base[1][:26] + b"CACACACACACA" + base[1][38:]]
    arms = [(m[:ARM], m[-ARM:]) for m in mols]
    L = Lane(rng)
    for M, unit in zip(mols, (1, 2)):
        for kind in ("del", "ins"):
            for size in (unit, 2 * unit):
                Mv = M[:30] + M[30 + size:] if kind == "del" else M[:30] + M[30:30 + size] + M[30:]
                variant(L, M, Mv, Mv, len(Mv), len(Mv), qual=ord("I"))
    got, want = session(acc, arms, L.shuffled())
    for W in (4, 15):
        counts, totals = compare(acc, got, want, mols, Ws=(W,))[(0, (1, 0), W)]
        assert totals["discordant"] == 0 and totals["ins_discordant"] == 0 and totals["gapped_sides"] == 16
        assert totals["deletions"] == (1 + 2) + (2 + 4)                                                         # the deleted bases, each once per molecule
        assert totals["insertions"] >= 4


# ---- quality and family ---------------------------------------------------------------------------------------------------------------------------------------
def test_quality_changes_the_counts_but_not_the_placement(acc, genome):
    rng = np.random.default_rng(479)
    mols, arms = cut_probes(genome, [90, 129])
    L = Lane(rng)
    for p, M in enumerate(mols):
        for k in range(6):
            Mv = plant(M, "del" if k % 2 else "ins", 30 + 5 * k, 1 + k % 3, rng)
            variant(L, M, Mv, Mv, len(Mv) - k, len(Mv) - 2 * k, family=1 + k % 2, qual=ord("I") if k % 3 == 0 else None)
    got, want = session(acc, arms, L.shuffled())
    res = compare(acc, got, want, mols, settings=((1, 0), (1, 40), (2, 0), (2, 40)), Ws=(4,))
    (c0, t0), (c40, t40) = res[(0, (1, 0), 4)], res[(0, (1, 40), 4)]
    assert np.array_equal(c0[:, 5:], c40[:, 5:]) and t0["gapped_sides"] == t40["gapped_sides"] and t0["deletions"] == t40["deletions"] > 0
    assert t40["bases"] < t0["bases"]
    assert res[(0, (2, 0), 4)][1]["used"] < t0["used"] and res[(0, (2, 0), 4)][1]["gapped_sides"] < t0["gapped_sides"]


# ---- molecules per cell -----------------------------------------------------------------------------------------------------------------------------------------
def test_molecules_per_cell(acc, genome):
    """Cells of 1, 4, threshold - 1, threshold and threshold + 1 molecules (one wavefront; a workgroup), a third of them with indels; an empty probe between
    populated ones."""
    rng = np.random.default_rng(487)
    sizes = [1, 4, 0, WG - 1, WG, WG + 1]
    mols, arms = cut_probes(genome, [40, 65, 40, 40, 40, 40])
    L = Lane(rng)
    for M, s in zip(mols, sizes):
        for k in range(s):
            if k % 3 == 0:
                Mv = plant(M, "del" if k % 2 else "ins", ARM + 1 + k % 3, 1 + k % 4, rng)
                variant(L, M, Mv, Mv if k % 9 else M, len(Mv) - k % 3, len(Mv) - k % 2, family=2 if k % 11 == 0 else 1, qual=ord("#") + (k % 3) * 19)
            else:
                L.molecule(M, len(M) - 3 * (k % 4), len(M) - 2 * (k % 3), qual=ord("#") + (k % 3) * 19)
    got, want = session(acc, arms, L.shuffled(), chunks=3)
    assert [sum(1 for g in got if g[0] == p) for p in range(len(sizes))] == sizes
    res = compare(acc, got, want, mols, settings=((1, 0), (2, 3)), Ws=(4,))
    counts, totals = res[(0, (1, 0), 4)]
    at = np.cumsum([0] + [len(m) for m in mols])
    assert not counts[at[2]:at[3]].any() and counts[at[5]:].any() and totals["groups"] == sum(sizes) and totals["gapped_sides"] > 300


# ---- rows ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_rows_and_independence_of_the_two_calls(acc, genome):
    """Two samples plus undetermined; rows out of order and one row twice; the ungapped call before and after the gapped one returns the same array."""
    rng = np.random.default_rng(491)
    mols, arms = cut_probes(genome, [90, 129, 64, 75])
    barcodes = draw_barcodes(rng, 2, 8)
    L = Lane(rng)
    for p, M in enumerate(mols):
        for k in range(4 + 2 * p):
            index = barcodes[k % 2] if k % 5 != 4 else random_tag(rng, 8)
            Mv = plant(M, "del" if k % 2 else "ins", ARM + 3 + 2 * k, 1 + k % 3, rng) if k % 3 else M
            variant(L, M, Mv, Mv, 70, 66, family=1 + k % 2, index=index)
    lens = [len(m) for m in mols]
    got, want = session(acc, arms, L.shuffled(), barcodes)
    assert {g[0] // len(arms) for g in got} == {0, 1, 2}
    before = [acc.consensus_pileup(lens, r) for r in range(3)]
    res = compare(acc, got, want, mols, rows=(2, 0, 1), settings=((1, 0), (2, 3)), Ws=(4,))
    assert sum(res[(r, (1, 0), 4)][1]["groups"] for r in range(3)) == len(got)
    for r in (2, 0, 1, 0, 0, 2):
        counts, totals = acc.consensus_pileup_gapped(mols, lens, r, max_indel=4)
        assert np.array_equal(counts, res[(r, (1, 0), 4)][0]) and totals == res[(r, (1, 0), 4)][1]
        plain = acc.consensus_pileup(lens, r)                                                                   # the two calls interleaved
        assert np.array_equal(plain[0], before[r][0]) and plain[1] == before[r][1]
        assert np.array_equal(plain[0], PR.pileup(want, lens, len(arms), r)[0])


def shared_frame_lane(rng, genome):
    """Two probes of 64 and 65 bases (one round; two, the second of one position); a cell above the workgroup threshold and a small one; a one-base deletion
    in six molecules of the first cell and two of the second."""
    mols, arms = cut_probes(genome, [64, 65])
    sizes = [WG + 1, 3]
    L = Lane(rng)
    for M, s in zip(mols, sizes):
        for k in range(s):
            if k % 50 == 1 or (s == 3 and k == 2):
                Mv = plant(M, "del", ARM + 5 + k % 20, 1, rng)
                variant(L, M, Mv, Mv, len(Mv), len(Mv))
            else:
                L.molecule(M, len(M), len(M) - 2 * (k % 3))
    return mols, arms, sizes, L.shuffled()


def test_the_two_tables_share_code_but_not_state(acc, genome):
    """One handle, the ungapped call, the gapped call, the ungapped call again: both ungapped tables are byte for byte the oracle's, the gapped table is its
    oracle's, totals included.  The cell of 257 molecules takes the workgroup frame in both instantiations, the cell of 3 the one-wavefront frame."""
    mols, arms, sizes, cols = shared_frame_lane(np.random.default_rng(509), genome)
    got, want = session(acc, arms, cols, chunks=2)
    assert got == want and [sum(1 for g in got if g[0] == p) for p in range(2)] == sizes
    lens = [len(m) for m in mols]
    first = acc.consensus_pileup(lens, 0)
    gapped = acc.consensus_pileup_gapped(mols, lens, 0, 1, 0, 4)
    again = acc.consensus_pileup(lens, 0)
    w_counts, w_totals = PR.pileup(want, lens, 2, 0)
    assert first[0].dtype == again[0].dtype == w_counts.dtype == np.int32
    assert first[0].tobytes() == again[0].tobytes() == w_counts.tobytes()
    assert first[1] == again[1] == w_totals
    g_counts, g_totals = G.pileup(want, mols, 2, 0, 1, 0, 4)
    assert gapped[0].dtype == np.int32 and gapped[0].tobytes() == g_counts.tobytes()
    assert gapped[1] == g_totals and tuple(gapped[1]) == KEYS
    assert g_totals["groups"] == WG + 4 and g_totals["deletions"] == 8 and g_totals["gapped_sides"] == 16 and w_totals["discordant"] > g_totals["discordant"] == 0


def test_the_substitution_only_lane(acc, genome):
    """On molecules with sparse substitutions only, columns 0-4 are the ungapped call's and columns 5-7 are zero."""
    rng = np.random.default_rng(457)
    mols, spec = substitution_lane(rng, genome)
    arms = [(m[:ARM], m[-ARM:]) for m in mols]
    L = Lane(rng)
    for k, (p, n_e, n_l, subs) in enumerate(spec):
        L.molecule(mols[p], n_e, n_l, family=1 + k % 2, subs=subs)
    got, want = session(acc, arms, L.shuffled())
    lens = [len(m) for m in mols]
    for W in (1, 4, 15):
        for mf, mq in ((1, 0), (2, 40)):
            counts, totals = compare(acc, got, want, mols, settings=((mf, mq),), Ws=(W,))[(0, (mf, mq), W)]
            plain, p_tot = acc.consensus_pileup(lens, 0, mf, mq)
            assert np.array_equal(counts[:, :5], plain) and not counts[:, 5:].any() and totals["gapped_sides"] == 0
            assert {k: totals[k] for k in p_tot} == p_tot


# ---- state, refusals, the untouched handle -----------------------------------------------------------------------------------------------------------------------
def test_state_refusals_and_a_plain_session_afterwards(genome):
    rng = np.random.default_rng(499)
    mols, arms = cut_probes(genome, [90, 64])
    L = Lane(rng)
    for M in mols:
        for k in range(3):
            Mv = plant(M, "del", 30 + k, 1 + k, rng)
            variant(L, M, Mv, Mv, 70, 66)
    ext, lig, eq, lq, idx = L.shuffled()
    n, lens = len(arms), np.array([len(m) for m in mols], dtype=np.int32)
    seq = b"".join(mols)
    a = _accel()
    try:
        lib, h = a.lib, a.h
        i32p = capi.C.POINTER(capi.C.c_int32)
        counts = np.full((int(lens.sum()), 8), -7, dtype=np.int32)
        tot = capi.GappedTotals()

        def call(seq_=seq, lens_=lens, n_=n, row=0, mf=1, mq=0, W=4, out=counts, tot_=tot):
            return lib.mipgen_accel_reads_consensus_pileup_gapped(h, seq_, lens_.ctypes.data_as(i32p) if lens_ is not None else None, n_, row, mf, mq, W,
                                                                  out.ctypes.data_as(i32p) if out is not None else None, capi.C.byref(tot_) if tot_ is not None else None)

        assert call() == E_STATE and b"holds no consensus reads" in lib.mipgen_accel_last_error()
        arr = capi.probe_array(arms)
        assert lib.mipgen_accel_reads_open_consensus(h, arr, n, 8, 0, 0, None, 0, 0, 0) == 0
        assert call() == E_STATE                                                                                # before the finish
        assert lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, None) == 0
        assert call() == 0 and not counts.any() and all(getattr(tot, k) == 0 for k in KEYS)                       # zero groups give zeros
        got = a.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=TAGS)[4]
        counts[:] = -7
        bad, long_ = lens.copy(), lens.copy()
        bad[1] = 0; long_[0] = 2049
        for kw in ({"seq_": None}, {"lens_": None}, {"n_": n - 1}, {"n_": n + 1}, {"lens_": bad}, {"lens_": long_}, {"row": -1}, {"row": 1}, {"mf": 0}, {"mq": -1},
                   {"mq": 41}, {"W": 0}, {"W": 16}, {"W": -1}):
            assert call(**kw) == E_INVALID, kw
        assert call(W=16) == E_INVALID and b"max_indel 16" in lib.mipgen_accel_last_error()
        assert call(lens_=long_) == E_INVALID and b"2048" in lib.mipgen_accel_last_error()
        assert (counts == -7).all()
        want_counts, want_totals = G.pileup(got, mols, n, 0, W=4)
        assert call() == 0 and np.array_equal(counts, want_counts) and {k: getattr(tot, k) for k in KEYS} == want_totals and want_totals["deletions"] == 12
        assert call(out=None) == 0 and tot.deletions == 12 and call(tot_=None) == 0 and np.array_equal(counts, want_counts)
        # timing: index 12 is this call's, index 11 stays the ungapped call's
        assert a.last_kernel_ms(12) < 0
        a.set_timing(True)
        a.consensus_pileup_gapped(mols, lens, max_indel=4)
        assert a.last_kernel_ms(12) > 0 and a.last_kernel_ms(11) < 0
        a.set_timing(False)
        # the next open drops the reads
        assert lib.mipgen_accel_reads_open(h, arr, n, 8, 0, 0) == 0
        assert call() == E_STATE
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
    """A small table cut from a golden genome on both strands and FASTQ with planted indels and substitutions: the file of -pileup_indels 4 byte for byte and
    both stderr lines; and -pileup without -pileup_indels, byte for byte what the ungapped oracle writes."""
    g = H.golden_genome()
    rng = np.random.default_rng(503 + with_barcodes)
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
        for k in range(3 + 3 * (p % 3)):
            tag = random_tag(rng, 8)
            Mv = M
            if k % 3 == 1:
                Mv = plant(M, "del", int(rng.integers(26, len(M) - 30)), 1 + k % 4, rng)
            elif k % 3 == 2:
                Mv = plant(M, "ins", int(rng.integers(26, len(M) - 26)), 1 + k % 3, rng)
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
    base = _run(common, str(tmp_path))
    assert base.returncode == 0, base.stderr.decode()
    # without -pileup_indels every byte is what it was
    text0, line0 = PR.pileup_file(want[4], t_rows, lab)
    p = _run(common + ["-pileup", "pile0.tsv"], str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert open(tmp_path / "pile0.tsv", "rb").read() == text0 and p.stderr.decode() == base.stderr.decode() + line0
    # with it
    text, lines = G.pileup_file(want[4], t_rows, lab, W=4)
    second = lines.split("\n")[1].split()
    assert int(second[4]) > 0 and int(second[6]) > 0 and b"\t-\t" in text and b"\t+\t" in text
    p = _run(common + ["-pileup", "pile.tsv", "-pileup_indels", "4"], str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert open(tmp_path / "pile.tsv", "rb").read() == text
    assert p.stderr.decode() == base.stderr.decode() + lines
    text2, lines2 = G.pileup_file(want[4], t_rows, lab, 2, 40, W=2)
    p = _run(common + ["-pileup", "pile2.tsv", "-pileup_indels", "2", "-pileup_min_family", "2", "-pileup_min_quality", "40"], str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert open(tmp_path / "pile2.tsv", "rb").read() == text2 != text and p.stderr.decode() == base.stderr.decode() + lines2
