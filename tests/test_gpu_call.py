"""GPU: variant calls end to end from reads (mipgen_accel_reads_consensus_call_pool / _consensus_call / _call_fetch, `mipgen_count -call`).  Planted
variants in lanes of two and three samples plus undetermined and without barcodes; every comparison is exact equality against tests/call_ref.py on the count
tables tests/pileup_ref.py / tests/gapped_ref.py make of the groups - the device's own fetched groups, which are asserted equal to those of tests/consensus_ref.py
from the reads - after the one exclusion of the model: a candidate whose exact score lies within 1e-6 of an integer is dropped from both sides, at most 1 in 1,000."""
import faulthandler
import json
import os

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CALL
from tests import consensus_ref as CR
from tests import gapped_ref as G
from tests import helpers as H
from tests import pileup_ref as PR
from tests import reads_ref as R
from tests.test_gpu_pileup import ARM, COUNT_BIN, TAGS, Lane, _run, cut_probes, session, write_fastq_q
from tests.test_gpu_reads import TABLES, _accel, random_tag
from tests.test_gpu_samples import GOLDEN_PLAIN, clean_reads_uneven_depth_inputs, draw_barcodes, plain_session_digest
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
    from mipgen_amd import synth
    return synth.random_genome(40000, 23)


def other(M, t, d=1):
    return b"ACGT"[(b"ACGT".index(M[t]) + d) & 3]


def tables_of(groups, mols, n_rows, W=0):
    """The count table of every row from the groups, by the pileup oracles."""
    lens, n = [len(m) for m in mols], len(mols)
    return [G.pileup(groups, mols, n, r, 1, 0, W)[0] if W else PR.pileup(groups, lens, n, r, 1, 0)[0] for r in range(n_rows)]


def check_row(acc, tables, pool, ref, row, n_sample, p, pileup):
    """consensus_call of one row, twice: its counts are the pileup call's, its records and totals the oracle's."""
    totals, cands = CALL.call_cells(tables[row], pool, ref, row < n_sample, p)
    assert totals["excluded"] * 1000 <= max(totals["candidates"], 1), (row, totals)
    counts, records, got_totals = acc.consensus_call(row, capi.CallParams(**p))
    counts2, records2, got_totals2 = acc.consensus_call(row, capi.CallParams(**p))
    assert np.array_equal(counts, counts2) and records.tobytes() == records2.tobytes() and got_totals == got_totals2
    assert np.array_equal(counts, tables[row]) and np.array_equal(counts, pileup(row)[0])
    assert {k: got_totals[k] for k in ("tested", "too_deep", "candidates")} == {k: totals[k] for k in ("tested", "too_deep", "candidates")}, row
    assert CALL.drop_excluded(records, cands) == CALL.kept_calls(cands, p), row
    assert totals["excluded"] or got_totals["calls"] == len(records) == totals["calls"]
    pt = acc.consensus_call_pileup_totals()
    want_pt = pileup(row)[1]
    assert {k: pt[k] for k in want_pt} == want_pt
    return [(int(r["pos"]), int(r["allele"])) for r in records]


def three_sample_lane(genome, rng):
    """Probes of 40, 77, 130 and 40 bases; three samples of 40 molecules per probe (the last probe: 257 in sample 0, a cell that takes a workgroup) and 10
    undetermined ones.  Probe 0, t 20: a substitution in 12 of sample 0's molecules.  Probe 1, t 30: the same substitution in 12 molecules of samples 0 AND 1.
    Probe 2, t 60: a substitution in ONE molecule of sample 2, of one read pair."""
    mols, arms = cut_probes(genome, [40, 77, 130, 40])
    barcodes = draw_barcodes(rng, 3, 8)
    L = Lane(rng)
    for s in range(4):
        index = barcodes[s] if s < 3 else None
        for p, M in enumerate(mols):
            for k in range(10 if s == 3 else 257 if (p, s) == (3, 0) else 40):
                subs = []
                if (p, s) == (0, 0) and k < 12:
                    subs = [(20, other(M, 20))]
                if p == 1 and s in (0, 1) and k < 12:
                    subs = [(30, other(M, 30, 2))]
                if (p, s, k) == (2, 2, 0):
                    subs = [(60, other(M, 60))]
                L.molecule(M, len(M), len(M), family=1 + (k % 3 == 0 and not subs), subs=subs, qual=ord("I"), index=index if index is not None else random_tag(rng, 8))
    return mols, arms, barcodes, L


def test_planted_substitutions_three_samples_and_the_background_filter(acc, genome):
    rng = np.random.default_rng(7401)
    mols, arms, barcodes, L = three_sample_lane(genome, rng)
    lens, ref = [len(m) for m in mols], b"".join(mols)
    got, want = session(acc, arms, L.shuffled(), barcodes, chunks=2)
    assert got == want and max(sum(1 for g in got if g[0] == c) for c in range(4)) == 257
    tables = tables_of(got, mols, 4)
    at = np.cumsum([0] + lens)
    before = [acc.consensus_pileup(lens, r) for r in range(4)]
    gapped_before = acc.consensus_pileup_gapped(mols, lens, 1, 1, 0, 4)
    pile = lambda row: before[row]
    site0, site1, site2 = (int(at[0]) + 20, b"ACGT".index(other(mols[0], 20))), (int(at[1]) + 30, b"ACGT".index(other(mols[1], 30, 2))), int(at[2]) + 60
    # a prior of 1 / 10: at 40 molecules a prior of 1,000 pseudo-observations would drown any background
    called = {}
    for bg in (200000, 10 ** 6):
        p = CALL.params(min_depth=20, min_alt=3, min_q=30, a0=1, n0=10, bg_max_ppm=bg)
        acc.consensus_call_pool(mols, lens, 1, 0, 0, bg)
        pool = CALL.pool(tables[:3], bg)
        for row in (2, 0, 1, 0, 3):                                                   # any order, a row twice, undetermined too
            called[(bg, row)] = check_row(acc, tables, pool, ref, row, 3, p, pile)
    assert called[(200000, 0)] == [site0, site1] and called[(200000, 1)] == [site1] and called[(200000, 2)] == [] and called[(200000, 3)] == []
    assert called[(10 ** 6, 0)] == [site0] and called[(10 ** 6, 1)] == [] and called[(10 ** 6, 2)] == []         # the carriers are now each other's background
    assert tables[2][site2].sum() == 40 and sorted(tables[2][site2][:4])[-2] == 1                                  # the single read pair: seen, and below min_alt
    # a pool remembers its bg_max_ppm
    lib, h = acc.lib, acc.h
    prm = capi.CallParams(bg_max_ppm=200000)
    tot = capi.CallTotals()
    assert lib.mipgen_accel_reads_consensus_call(h, 0, capi.C.byref(prm), None, capi.C.byref(tot)) == E_STATE and b"the pool was built with 1000000" in lib.mipgen_accel_last_error()
    prm = capi.CallParams(bg_max_ppm=10 ** 6, a0=1, n0=10)
    assert lib.mipgen_accel_reads_consensus_call(h, 0, capi.C.byref(prm), None, None) == 0                         # counts and totals may both be NULL
    for bad_row in (-1, 4):
        assert lib.mipgen_accel_reads_consensus_call(h, bad_row, capi.C.byref(prm), None, None) == E_INVALID
    prm.min_alt = 0
    assert lib.mipgen_accel_reads_consensus_call(h, 0, capi.C.byref(prm), None, None) == E_INVALID
    # the two pileup calls return what they returned before the pool
    for r in range(4):
        counts, totals = acc.consensus_pileup(lens, r)
        assert np.array_equal(counts, before[r][0]) and totals == before[r][1]
    again = acc.consensus_pileup_gapped(mols, lens, 1, 1, 0, 4)
    assert np.array_equal(again[0], gapped_before[0]) and again[1] == gapped_before[1]


def test_a_deletion_of_two_bases_two_samples(acc, genome):
    """max_indel 4: a deletion of 2 bases in 8 of sample 0's 25 molecules is called as del on both positions, there and nowhere else; the counts are the gapped
    pileup's.  Two samples plus undetermined."""
    rng = np.random.default_rng(7411)
    mols, arms = cut_probes(genome, [40, 64])
    barcodes = draw_barcodes(rng, 2, 8)
    L = Lane(rng)
    t = 24
    M1 = mols[1]
    while M1[t] == M1[t + 2] or M1[t + 1] == M1[t + 3] or M1[t - 1] == M1[t + 1]:    # (a deletion that can slide along a repeat has no single placement to assert below)
        t += 1
    deleted = M1[:t] + M1[t + 2:]
    for s in range(3):
        for p, M in enumerate(mols):
            for k in range(6 if s == 2 else 25):
                index = barcodes[s] if s < 2 else random_tag(rng, 8)
                if (p, s) == (1, 0) and k < 8:
                    L.molecule(M, len(M), len(M), qual=ord("I"), index=index,
                               member_edit=lambda m, e, l, eq, lq: (e[:TAGS[0]] + deleted, R.revcomp(deleted), b"I" * (TAGS[0] + len(deleted)), b"I" * len(deleted)))
                else:
                    L.molecule(M, len(M), len(M), qual=ord("I"), index=index)
    got, want = session(acc, arms, L.shuffled(), barcodes)
    lens, ref = [len(m) for m in mols], b"".join(mols)
    tables = tables_of(got, mols, 3, W=4)
    p = CALL.params(min_depth=20, min_alt=3, min_q=30)
    acc.consensus_call_pool(mols, lens, 1, 0, 4, p["bg_max_ppm"])
    pool = CALL.pool(tables[:2], p["bg_max_ppm"])
    pile = lambda row: acc.consensus_pileup_gapped(mols, lens, row, 1, 0, 4)
    calls = {row: check_row(acc, tables, pool, ref, row, 2, p, pile) for row in (1, 0, 2)}
    assert calls[0] == [(40 + t, 4), (40 + t + 1, 4)] and calls[1] == [] and calls[2] == []
    assert tables[0][40 + t][5] == 8 == tables[0][40 + t + 1][5]


def test_without_barcodes_the_one_row_is_called_against_the_prior(acc, genome):
    rng = np.random.default_rng(7421)
    mols, arms = cut_probes(genome, [130, 41])
    L = Lane(rng)
    for p, M in enumerate(mols):
        for k in range(30):
            L.molecule(M, 70, 66, family=1 + k % 2, subs=[(50, other(M, 50))] if p == 0 and k < 9 else [], err=0.01)
    got, want = session(acc, arms, L.shuffled())
    lens, ref = [len(m) for m in mols], b"".join(mols)
    tables = tables_of(got, mols, 1)
    p = CALL.params(min_depth=10, min_alt=3, min_q=30)
    acc.consensus_call_pool(mols, lens, 1, 0, 0, p["bg_max_ppm"])
    pool = CALL.pool(tables, p["bg_max_ppm"])
    calls = check_row(acc, tables, pool, ref, 0, 1, p, lambda row: acc.consensus_pileup(lens, row))
    assert (50, b"ACGT".index(other(mols[0], 50))) in calls
    records = acc.consensus_call(0, capi.CallParams(**p))[1]
    hit = records[records["pos"] == 50][0]
    assert (hit["alt"], hit["bg_alt"]) == (9, 0) and hit["bg_depth"] == 0            # 9 of 30 is above bg_max_ppm: the row was never in its own background


def test_state_and_a_plain_session_afterwards(genome):
    rng = np.random.default_rng(7431)
    mols, arms = cut_probes(genome, [64, 90])
    lens = np.array([64, 90], dtype=np.int32)
    seq = b"".join(mols)
    L = Lane(rng)
    for p, M in enumerate(mols):
        for k in range(25):
            L.molecule(M, 60, 60, subs=[(30, other(M, 30))] if k < 8 else [])
    ext, lig, eq, lq, idx = L.shuffled()
    a = _accel()
    try:
        lib, h, C = a.lib, a.h, capi.C
        i32p = C.POINTER(C.c_int32)
        prm, tot = capi.CallParams(), capi.CallTotals()
        pool = lambda seq_=seq, lens_=lens, n=2, mf=1, mq=0, W=0, bg=200000: lib.mipgen_accel_reads_consensus_call_pool(
            h, seq_, lens_.ctypes.data_as(i32p) if lens_ is not None else None, n, mf, mq, W, bg)
        call = lambda row=0: lib.mipgen_accel_reads_consensus_call(h, row, C.byref(prm), None, C.byref(tot))
        # nothing is held
        assert pool() == E_STATE and call() == E_STATE and b"holds no consensus reads" in lib.mipgen_accel_last_error()
        assert lib.mipgen_accel_reads_consensus_call_pileup_totals(h, None) == E_STATE
        a.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=TAGS)
        # reads but no pool
        assert call() == E_STATE and b"have no pool" in lib.mipgen_accel_last_error()
        # every refusal of the pool, and none of them leaves one
        long_lens = np.array([64, 3000], dtype=np.int32)
        for kw in (dict(seq_=None), dict(lens_=None), dict(n=1), dict(n=3), dict(mf=0), dict(mq=41), dict(mq=-1), dict(W=-1), dict(W=16), dict(bg=-1), dict(bg=10 ** 6 + 1),
                   dict(lens_=np.array([64, 0], dtype=np.int32)), dict(lens_=long_lens, seq_=b"A" * 3064, W=4)):
            assert pool(**kw) == E_INVALID, kw
            assert call() == E_STATE
        assert pool(lens_=long_lens, seq_=b"A" * 3064) == 0                           # (only the gapped table bounds the molecule length)
        assert pool() == 0 and call() == 0 and tot.calls == 2
        assert call(1) == E_INVALID and b"row 1" in lib.mipgen_accel_last_error()     # one row without barcodes
        assert a.last_kernel_ms(13) < 0
        a.set_timing(True)
        assert pool() == 0 and a.last_kernel_ms(13) > 0
        assert call() == 0 and a.last_kernel_ms(13) > 0 and a.last_kernel_ms(11) < 0 and a.last_kernel_ms(12) < 0
        a.set_timing(False)
        records = a.call_fetch(2)
        assert records["pos"].tolist() == [30, 64 + 30] and (records["alt"] == 8).all()
        # the next open drops reads and pool; the records of the last call stay fetchable
        arr = capi.probe_array(arms)
        assert lib.mipgen_accel_reads_open_consensus(h, arr, 2, 8, 0, 0, None, 0, 0, 0) == 0
        assert call() == E_STATE and pool() == E_STATE
        assert lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, None) == 0
        assert call() == E_STATE and b"have no pool" in lib.mipgen_accel_last_error()
        assert pool() == 0 and call() == 0 and (tot.tested, tot.candidates, tot.calls) == (0, 0, 0)      # a session without groups: zero tables, nothing tested
    finally:
        a.close()


@pytest.mark.parametrize("name,key", TABLES[:1])
def test_a_plain_session_afterwards_is_the_recorded_one(acc, genome, name, key):
    rng = np.random.default_rng(7441)
    mols, arms = cut_probes(genome, [64, 90])
    L = Lane(rng)
    for M in mols:
        for k in range(22):
            L.molecule(M, 60, 60)
    ext, lig, eq, lq, idx = L.shuffled()
    acc.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=TAGS)
    acc.consensus_call_pool(mols, [64, 90])
    acc.consensus_call(0, capi.CallParams())
    t_rows, t_ext, t_lig = clean_reads_uneven_depth_inputs(name, key)
    got = acc.count_reads([(r[6], r[10]) for r in t_rows], t_ext, t_lig, want_assignment=True)
    recorded = json.load(open(GOLDEN_PLAIN))
    assert plain_session_digest(*got) == recorded[f"{name}/{key}"]["sha256"]


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("indels", [0, 4])
@pytest.mark.parametrize("with_barcodes", [False, True])
def test_cli_equals_the_oracle(tmp_path, with_barcodes, indels):
    """A table cut from a golden genome on both strands, FASTQ with planted substitutions and (for -pileup_indels) deletions: CALLS byte for byte what
    call_ref.calls_file writes, FILE byte for byte what it is without -call, and the new last stderr line."""
    g = H.golden_genome()
    rng = np.random.default_rng(7450 + 2 * with_barcodes + (indels > 0))
    t_rows, at = [], 5000
    for k in range(4):
        first = clean_window(g, at, 140)
        length = (64, 90, 130, 70)[k]
        t_rows.append(synthetic_row(g, first, first + length - 1, b"+" if k % 2 else b"-", arm=16 + k))
        at = first + 400
    with open(tmp_path / "table.txt", "wb") as fh:
        fh.write(HEADER.encode() + b"".join(b"\t".join(r) + b"\n" for r in t_rows))
    mols = [r[6] + r[13] + r[10] for r in t_rows]
    arms = [(r[6], r[10]) for r in t_rows]
    barcodes = draw_barcodes(rng, 3, 8)
    labels = ["sample_a", "sample_b", "sample_c"]
    ext, lig, eq, lq, idx = [], [], [], [], []
    for p, M in enumerate(mols):
        for s in range(3):
            for k in range(3 if s == 2 else 14):
                tag = random_tag(rng, 8)
                Mv = bytearray(M)
                t = 24 + 3 * p + s
                if k < 5 and s == 0:
                    Mv[t] = other(M, t, 1 + p % 3)                                    # a variant of sample_a
                if k in (5, 6, 7) and s <= 1:
                    Mv[t + 4] = other(M, t + 4, 2)                                    # one that both samples carry, at 3 of 14
                if indels and k >= 10 and s == 1 and p % 2 == 0:
                    del Mv[30 + p:32 + p]                                             # a deletion of two bases in sample_b
                index = barcodes[s] if s < 2 else random_tag(rng, 8)
                e = tag[:5] + (bytes(Mv) + b"GATTACAGATTACAGATTACA" * 8)[:95]
                l = tag[5:] + (R.revcomp(bytes(Mv)) + b"CTTCAGCTTCCCGATATCCGA" * 8)[:97]
                ext.append(e); lig.append(l); idx.append(index)
                eq.append(rng.integers(35, 75, len(e)).astype(np.uint8).tobytes()); lq.append(rng.integers(35, 75, len(l)).astype(np.uint8).tobytes())
    write_fastq_q(tmp_path / "ext.fq", ext, eq); write_fastq_q(tmp_path / "lig.fq", lig, lq)
    write_fastq_q(tmp_path / "i1.fq", idx, [b"I" * 8] * len(idx))
    with open(tmp_path / "samples.tsv", "wb") as fh:
        fh.write(b"\n".join(l.encode() + b"\t" + b for l, b in zip(labels, barcodes)) + b"\n")
    common = [COUNT_BIN, "-tag_sizes", "5,3", "-reads", "ext.fq", "lig.fq", "table.txt", "-o", "counts.tsv"] + (
        ["-barcodes", "samples.tsv", "-index_reads", "i1.fq"] if with_barcodes else [])
    pile_args = ["-pileup_indels", str(indels)] if indels else []
    want = CR.consensus_reads(arms, ext, lig, eq, lq, idx if with_barcodes else None, barcodes if with_barcodes else None, 0, (5, 3))
    assert want[2]["assigned"] == len(ext)
    lab = labels if with_barcodes else None
    tables = tables_of(want[4], mols, 4 if with_barcodes else 1, W=indels)
    p = CALL.params(min_depth=10, min_alt=3, min_ppm=50000, min_q=20, a0=1, n0=200, bg_max_ppm=250000)
    text, line, excluded = CALL.calls_file(tables, t_rows, lab, p)
    assert excluded == 0 and text.count(b"\n") >= (4 if with_barcodes else 2) and b"\t-\t" in text and b"\t+\t" in text
    if indels and with_barcodes:
        assert any(l.split(b"\t")[7] == b"-" for l in text.split(b"\n")[1:-1])       # a called deletion
    plain = _run(common + ["-pileup", "pile0.tsv"] + pile_args, str(tmp_path))
    assert plain.returncode == 0, plain.stderr.decode()
    call_args = ["-call_min_depth", "10", "-call_min_alt", "3", "-call_min_ppm", "50000", "-call_min_q", "20", "-call_prior", "1,200", "-call_background_max_ppm", "250000"]
    both = _run(common + ["-pileup", "pile.tsv", "-call", "calls.tsv"] + pile_args + call_args, str(tmp_path))
    assert both.returncode == 0, both.stderr.decode()
    assert open(tmp_path / "calls.tsv", "rb").read() == text
    assert open(tmp_path / "pile.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read() != b""
    assert both.stderr.decode() == plain.stderr.decode() + line and both.stdout == plain.stdout
    if not indels and not with_barcodes:                                              # the defaults are the documented ones
        default = _run(common + ["-pileup", "pile1.tsv", "-call", "calls1.tsv"], str(tmp_path))
        text1, line1, _ = CALL.calls_file(tables, t_rows, lab, CALL.params())
        assert default.returncode == 0 and open(tmp_path / "calls1.tsv", "rb").read() == text1 and default.stderr.decode() == plain.stderr.decode() + line1
