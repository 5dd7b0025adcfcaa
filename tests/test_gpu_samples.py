"""GPU: reads and unique tags per probe AND per sample of a multiplexed lane (mipgen_accel_reads_open_samples / _feed_samples / _finish_samples /
_last_samples, `mipgen_count -barcodes`).  Every case is held, by exact equality, against tests/samples_ref.py - every index against every
barcode, every pair against every probe - and against a plain session on the same pairs: the probe of a pair, the six totals and the column sums of
`reads` do not depend on the samples.  Probes are rows of the committed golden MIP tables; pairs and indices come from seeded generators."""
import faulthandler
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi, synth
from tests import helpers as H
from tests import reads_ref as R
from tests import samples_ref as SR
from tests.test_gpu_reads import BASES, TABLES, _accel, _mixed_reads, _subset_table, arms_of, random_tag, read_pair, substitute, table_rows, write_fastq

pytestmark = pytest.mark.gpu
COUNT_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_count")
GOLDEN_PLAIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reads_plain_sessions.json")
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


def draw_barcodes(rng, n, J, min_dist=3):
    """n barcodes of J bases, pairwise at least min_dist apart: random draws, one kept when it is far enough from all that were kept."""
    kept = np.zeros((0, J), dtype=np.uint8)
    while len(kept) < n:
        c = BASES[rng.integers(0, 4, J)]
        if len(kept) == 0 or int((kept != c[None, :]).sum(axis=1).min()) >= min_dist:
            kept = np.vstack([kept, c[None, :]])
    return [k.tobytes() for k in kept]


def lane(rows, barcodes, rng, te, tl, n_pairs, index_errors=0.03, tags_per_probe=0):
    """A multiplexed lane: pairs of random probes of `rows`, every pair with the index of a sample drawn at uneven depth (some samples get nothing);
    a fraction of the indices with one substitution, a few random ones, and bases beyond the barcode on every other index."""
    n_s = len(barcodes)
    w = rng.random(n_s) ** 3 * (rng.random(n_s) > 0.15)
    w[0] += 1e-3
    w = w / w.sum()
    ext, lig, idx = [], [], []
    pool = {p: [random_tag(rng, te + tl) for _ in range(tags_per_probe)] for p in range(len(rows))} if tags_per_probe else None
    for _ in range(n_pairs):
        p = int(rng.integers(0, len(rows)))
        tag = pool[p][int(rng.integers(0, tags_per_probe))] if pool and rng.random() < 0.8 else None
        e, l = read_pair(rows[p], rng, te, tl, tag=tag)
        i = barcodes[int(rng.choice(n_s, p=w))]
        u = rng.random()
        if u < index_errors:
            i = substitute(i, int(rng.integers(0, len(i))), rng)
        elif u < index_errors + 0.01:
            i = random_tag(rng, len(i))
        if rng.random() < 0.5:
            i = i + random_tag(rng, int(rng.integers(1, 5)))
        ext.append(e); lig.append(l); idx.append(i)
    return ext, lig, idx


def check(acc, arms, ext, lig, idx, barcodes, d, tag_sizes=(5, 0), mismatches=0, swap_reads=False, chunks=1, key_buffer=0, plain=True):
    """The device against the oracle - both matrices, row_pairs, the eight totals, the sample and the probe of every pair - and against a plain session."""
    want = SR.count_reads_samples(arms, ext, lig, idx, barcodes, d, tag_sizes, mismatches, swap_reads)
    got = acc.count_reads_samples(arms, ext, lig, idx, barcodes, d, tag_sizes, mismatches, swap_reads, chunks, key_buffer, want_assignment=True)
    reads, unique, tot, row_pairs, sample, probe = got
    assert np.array_equal(sample, want[4]), f"first pair whose sample differs: {int(np.flatnonzero(sample != want[4])[0])}"
    assert np.array_equal(probe, want[5]), f"first pair whose probe differs: {int(np.flatnonzero(probe != want[5])[0])}"
    assert reads.shape == want[0].shape == (len(barcodes) + 1, len(arms))
    assert np.array_equal(reads, want[0]) and np.array_equal(unique, want[1])
    assert np.array_equal(row_pairs, want[3]) and int(row_pairs.sum()) == len(ext)
    assert tot == want[2], (tot, want[2])
    assert int(row_pairs[-1]) == tot["sample_none"] + tot["sample_ambiguous"]
    if plain:
        p_reads, p_unique, p_tot, p_assign = acc.count_reads(arms, ext, lig, tag_sizes, mismatches, swap_reads, want_assignment=True)
        assert np.array_equal(reads.sum(axis=0), p_reads) and np.array_equal(probe, p_assign)
        assert (unique.sum(axis=0) >= p_unique).all()
        assert {k: tot[k] for k in p_tot} == p_tot
    return got


CLEAN = [("svr_small", "all_mips", 6, 3), ("svr_2kb", "picked_mips", 8, 96), ("long_capture_svr", "picked_mips", 16, 1536), ("logistic_snp_trf", "all_mips", 32, 1),
         ("svr_small", "all_mips", 32, 96)]


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("name,key,J,n_samples", CLEAN)
def test_clean_runs(acc, name, key, J, n_samples, d):
    """The four golden tables; indices of 6, 8, 16 and 32 bases; 1, 3, 96 and 1,536 samples at uneven depth."""
    assert (name, key) in TABLES
    rows = table_rows(name, key)
    rng = np.random.default_rng(101 + J + n_samples)
    barcodes = draw_barcodes(rng, n_samples, J)
    assert len(barcodes) == n_samples and (n_samples == 1 or SR.min_pairwise_distance(barcodes) >= 3)
    ext, lig, idx = lane(rows, barcodes, rng, 5, 0, 24000, tags_per_probe=6)
    reads, unique, tot, row_pairs, sample, _ = check(acc, arms_of(rows), ext, lig, idx, barcodes, d)
    assert tot["sample_ambiguous"] == 0                                       # it cannot tie at d = 0, nor at d = 1 with barcodes >= 3 apart
    assert tot["assigned"] > 0 and tot["sample_none"] > (0 if d else 500), tot
    if n_samples >= 96:
        assert (row_pairs[:-1] == 0).any() and row_pairs[:-1].max() > 4 * np.median(row_pairs[:-1])      # uneven depth
    elif n_samples > 1:
        assert len(set(row_pairs[:-1].tolist())) == n_samples
    if d == 1:
        # every index one substitution from its barcode found its sample: what is left is the random ones
        assert tot["sample_none"] < 24000 * 0.02


@pytest.mark.parametrize("tag_sizes", [(5, 0), (4, 3), (0, 0), (8, 8)])
def test_shared_tags(acc, tag_sizes):
    """The same tag on the same probe in two samples is a molecule in each; read twice in one sample it is one."""
    te, tl = tag_sizes
    rows = table_rows("svr_small", "all_mips", 120)[::3]
    rng = np.random.default_rng(7)
    barcodes = draw_barcodes(rng, 3, 8)
    shared = [random_tag(rng, te + tl) for _ in range(3)]
    ext, lig, idx = [], [], []
    for r in rows:
        for t in shared + [random_tag(rng, te + tl) for _ in range(int(rng.integers(0, 4)))]:
            for s in (0, 1, 1, 2, 2, 2)[:int(rng.integers(2, 7))]:
                e, l = read_pair(r, rng, te, tl, tag=t)
                ext.append(e); lig.append(l); idx.append(barcodes[s])
    reads, unique, tot, _, _, _ = check(acc, arms_of(rows), ext, lig, idx, barcodes, 0, tag_sizes)
    p_reads, p_unique, _ = acc.count_reads(arms_of(rows), ext, lig, tag_sizes)
    if te + tl == 0:
        assert np.array_equal(unique, reads)
    else:
        seen = np.flatnonzero(p_reads)
        assert len(seen) > 10 and (unique[0, seen] >= 3).all() and (unique[1, seen] >= 3).all()
        assert (unique.sum(axis=0)[seen] >= 2 * p_unique[seen]).all()         # every tag was read in samples 0 and 1: two molecules, one plain group
        assert (unique[1] < reads[1]).any()


NEAR = [b"AAAAAAAA", b"AAAAAAAC", b"GGGGGGGG", b"GGGGGGTT", b"CCCCTTTT", b"TTTTCCCC"]          # a pair at distance 1, a pair at distance 2, the rest far


def _index_variants(rng, bc):
    q = sorted(rng.choice(len(bc), 2, replace=False).tolist())
    one = substitute(bc, q[0], rng)
    return [bc, one, substitute(one, q[1], rng), bc[:q[0]] + b"N" + bc[q[0] + 1:], bc[:q[0]] + b"N" + bc[q[0] + 1:q[1]] + b"N" + bc[q[1] + 1:],
            bc[:q[1]] + bc[q[1]:q[1] + 1].lower() + bc[q[1] + 1:], bc.lower(), bc[:-1], b"", bc + b"ACGT", substitute(bc, len(bc) - 1, rng) + b"NN",
            bc[:q[0]] + b"N" + substitute(bc, q[1], rng)[q[0] + 1:], b"N" * len(bc), bc[:q[0]] + b"." + bc[q[0] + 1:]]


@pytest.mark.parametrize("m", [0, 1, 2])
@pytest.mark.parametrize("d", [0, 1])
def test_index_errors_and_arm_errors(acc, d, m):
    """One and two substitutions, N and lower case, short and empty indices - on barcodes >= 3 apart and on a set with a pair at distance 1 and a pair
    at distance 2 - together with substitutions in the arms at every allowed mismatch count."""
    rows = [r for r in table_rows("svr_small", "all_mips", 200)[::4] if min(len(r[6]), len(r[10])) > 16]
    arms = arms_of(rows)
    rng = np.random.default_rng(300 + 10 * d + m)
    far = draw_barcodes(rng, 12, 8, min_dist=5)                             # (two substitutions leave an index >= 3 from every other barcode)
    for barcodes in (far, NEAR):
        ext, lig, idx = [], [], []
        for k, r in enumerate(rows):
            for v, i in enumerate(_index_variants(rng, barcodes[k % len(barcodes)])):
                e, l = read_pair(r, rng, 5, 2)
                if v % 4 == 1:
                    e = substitute(e, 5 + int(rng.integers(0, len(r[6]))), rng)
                elif v % 4 == 2:
                    l = substitute(l, 2 + int(rng.integers(0, len(r[10]))), rng)
                    e = substitute(e, 5 + len(r[6]) - 1, rng)
                elif v % 4 == 3 and v > 8:
                    e = e[:6] + b"N" + e[7:]
                ext.append(e); lig.append(l); idx.append(i)
        # between the pair at distance 2, on the pair at distance 1, and next to it
        for i in (b"GGGGGGGT", b"GGGGGGTG", b"GGGGGGNT", b"GGGGGGTN", b"AAAAAAAC", b"AAAAAAAA", b"AAAAAAAG", b"AAAAAAAN", b"CAAAAAAA", b"CAAAAAAC", b"NAAAAAAC"):
            e, l = read_pair(rows[0], rng, 5, 2)
            ext.append(e); lig.append(l); idx.append(i)
        _, _, tot, _, sample, _ = check(acc, arms, ext, lig, idx, barcodes, d, (5, 2), m)
        tail = sample[-11:].tolist()
        if barcodes is NEAR:
            assert tail == ([-1, -1, -1, -1, 1, 0, -1, -1, -1, -1, -1] if d == 0 else [-2, -2, 3, 3, 1, 0, -2, -2, 0, 1, 1])
            assert (tot["sample_ambiguous"] > 0) == (d == 1)
        else:
            assert tot["sample_ambiguous"] == 0
        by_variant = sample[:-11].reshape(len(rows), 14)
        assert (by_variant[:, 0] >= 0).all() and (by_variant[:, 9] >= 0).all()
        assert (by_variant[:, [4, 6, 7, 8, 12]] == SR.NONE).all()
        if barcodes is far:
            assert (by_variant[:, 2] == SR.NONE).all()
            assert ((by_variant[:, [1, 3, 5, 10, 13]] >= 0) == (d == 1)).all() and (by_variant[:, 11] == SR.NONE).all()


def test_chunks_and_key_buffer_do_not_change_the_result(acc):
    rows = table_rows("logistic_snp_trf", "all_mips", 300)
    rng = np.random.default_rng(43)
    barcodes = draw_barcodes(rng, 96, 8)
    ext, lig, idx = lane(rows, barcodes, rng, 4, 4, 30000, tags_per_probe=5)
    first = check(acc, arms_of(rows), ext, lig, idx, barcodes, 1, (4, 4), 1)
    for chunks, key_buffer in [(3, 0), (17, 0), (1, 256), (3, 3000), (17, 1)]:
        got = acc.count_reads_samples(arms_of(rows), ext, lig, idx, barcodes, 1, (4, 4), 1, chunks=chunks, key_buffer=key_buffer, want_assignment=True)
        assert all(np.array_equal(g, f) for g, f in zip(got[:2] + got[3:], first[:2] + first[3:])) and got[2] == first[2], (chunks, key_buffer)


def test_refusals_state_and_untouched_handle():
    """Every refusal of open_samples with its code, feed / finish of the wrong kind (the session then completes correctly), and the handle's dense
    results unchanged after each refused call and after a session."""
    genome = synth.random_genome(12000, 5)
    P = capi.make_params(130, 140, score_method=capi.SCORE_LOGISTIC, arm_pairs=synth.arm_pairs_from_sums([43, 44]))
    a = capi.Accel(P)
    try:
        a.upload([capi.build_region(genome, "1", 5000, 5055, P, bwa_mode="hashed", label="s1")])
        a.score_resident(capi.SCORE_LOGISTIC)
        s0, r0 = a.download()

        def unchanged():
            s, r = a.download()
            assert np.array_equal(s.view(np.int64), s0.view(np.int64)) and np.array_equal(r, r0)

        rows = table_rows("svr_small", "all_mips", 80)
        arms = arms_of(rows)
        rng = np.random.default_rng(47)
        barcodes = draw_barcodes(rng, 5, 8)
        ext, lig, idx = lane(rows, barcodes, rng, 5, 0, 3000, tags_per_probe=3)
        want = check(a, arms, ext, lig, idx, barcodes, 1)
        unchanged()
        lib, h = a.lib, a.h
        i64p, i32p = capi.C.POINTER(capi.C.c_int64), capi.C.POINTER(capi.C.c_int32)
        arr, bc = capi.probe_array(arms), capi.c_strings(barcodes)
        n, ns = len(arms), len(barcodes)
        open_s = lib.mipgen_accel_reads_open_samples
        one = np.zeros(2, dtype=np.int64)
        op = one.ctypes.data_as(i64p)
        # nothing is open
        assert lib.mipgen_accel_reads_feed_samples(h, 1, b"A", op, b"A", op, b"A", op) == E_STATE
        assert lib.mipgen_accel_reads_finish_samples(h, None, None, None, None, None) == E_STATE
        assert lib.mipgen_accel_reads_last_samples(h, np.zeros(1, dtype=np.int32).ctypes.data_as(i32p), 1) == E_STATE; unchanged()
        # everything the plain open refuses
        assert open_s(h, None, n, 5, 0, 0, bc, ns, 0) == E_INVALID
        assert open_s(h, arr, 0, 5, 0, 0, bc, ns, 0) == E_INVALID
        assert open_s(h, arr, n, 9, 8, 0, bc, ns, 0) == E_INVALID
        assert open_s(h, arr, n, -1, 0, 0, bc, ns, 0) == E_INVALID
        assert open_s(h, arr, n, 5, 0, 3, bc, ns, 0) == E_INVALID
        assert open_s(h, capi.probe_array([(b"ACGTACGTACG", b"ACGTACGTACGTACGTAA")]), 1, 5, 0, 0, bc, ns, 0) == E_INVALID and b"12" in lib.mipgen_accel_last_error()
        assert open_s(h, capi.probe_array([(b"", b"ACGTACGTACGTACGTAA")]), 1, 5, 0, 0, bc, ns, 0) == E_INVALID
        assert open_s(h, capi.probe_array([(b"ACGTACGTACGTACGTAA", None)]), 1, 5, 0, 0, bc, ns, 0) == E_INVALID
        assert open_s(h, capi.probe_array([(b"ACGT" * 17, b"ACGTACGTACGTACGTAA")]), 1, 5, 0, 0, bc, ns, 0) == E_INVALID; unchanged()
        # and what the barcodes add
        assert open_s(h, arr, n, 5, 0, 0, None, ns, 0) == E_INVALID
        assert open_s(h, arr, n, 5, 0, 0, bc, 0, 0) == E_INVALID
        assert open_s(h, arr, n, 5, 0, 0, capi.c_strings([b"ACGTACGT", None]), 2, 0) == E_INVALID
        assert open_s(h, arr, n, 5, 0, 0, capi.c_strings([b"ACGTACGT", b"ACGTACG"]), 2, 0) == E_INVALID and b"unequal length" in lib.mipgen_accel_last_error()
        assert open_s(h, arr, n, 5, 0, 0, capi.c_strings([b""]), 1, 0) == E_INVALID
        assert open_s(h, arr, n, 5, 0, 0, capi.c_strings([b"ACGTACGN"]), 1, 0) == E_INVALID and b"A C G T" in lib.mipgen_accel_last_error()
        assert open_s(h, arr, n, 5, 0, 0, capi.c_strings([b"ACGTACGt"]), 1, 0) == E_INVALID
        assert open_s(h, arr, n, 5, 0, 0, capi.c_strings([b"ACGTACGT", b"TTTTACGT", b"ACGTACGT"]), 3, 0) == E_INVALID and b"twice" in lib.mipgen_accel_last_error()
        assert open_s(h, arr, n, 5, 0, 0, capi.c_strings([b"ACGT" * 8 + b"A"]), 1, 0) == E_INVALID
        assert open_s(h, arr, n, 5, 0, 0, bc, ns, 2) == E_INVALID
        assert open_s(h, arr, n, 5, 0, 0, bc, ns, -1) == E_INVALID; unchanged()
        # (n_samples + 1) * n > 2^32: every barcode of 8 bases and 65,536 probes
        every = [bytes(BASES[[(k >> (2 * j)) & 3 for j in range(8)]]) for k in range(65536)]
        many = capi.probe_array([arms[0]] * 65536)
        assert open_s(h, many, 65536, 5, 0, 0, capi.c_strings(every), 65536, 0) == E_INVALID and b"2^32" in lib.mipgen_accel_last_error(); unchanged()

        # the wrong kind: refused, the session left as it was, and it completes correctly
        (eb, eo), (lb, lo), (ib, io) = capi.pack_reads(ext), capi.pack_reads(lig), capi.pack_reads(idx)
        half = len(ext) // 2
        feed_s = lambda x, y: lib.mipgen_accel_reads_feed_samples(h, y - x, eb[eo[x]:].ctypes.data, eo[x:y + 1].ctypes.data_as(i64p), lb[lo[x]:].ctypes.data,
                                                                  lo[x:y + 1].ctypes.data_as(i64p), ib[io[x]:].ctypes.data, io[x:y + 1].ctypes.data_as(i64p))
        feed_p = lambda x, y: lib.mipgen_accel_reads_feed(h, y - x, eb[eo[x]:].ctypes.data, eo[x:y + 1].ctypes.data_as(i64p), lb[lo[x]:].ctypes.data,
                                                          lo[x:y + 1].ctypes.data_as(i64p))
        assert open_s(h, arr, n, 5, 0, 0, bc, ns, 1) == 0
        assert open_s(h, arr, n, 5, 0, 0, bc, ns, 1) == E_STATE and lib.mipgen_accel_reads_open(h, arr, n, 5, 0, 0) == E_STATE
        assert feed_s(0, half) == 0
        assert feed_p(half, len(ext)) == E_STATE
        assert lib.mipgen_accel_reads_finish(h, None, None, None) == E_STATE; unchanged()
        bad = np.array([0, 5, 3], dtype=np.int64)
        good = np.array([0, 4, 8], dtype=np.int64)
        gp, bp = good.ctypes.data_as(i64p), bad.ctypes.data_as(i64p)
        assert lib.mipgen_accel_reads_feed_samples(h, 2, b"AAAAAAAA", gp, b"AAAAAAAA", gp, b"AAAAAAAA", bp) == E_INVALID and b"index offsets" in lib.mipgen_accel_last_error()
        assert lib.mipgen_accel_reads_feed_samples(h, 2, b"AAAAAAAA", gp, b"AAAAAAAA", gp, None, gp) == E_INVALID; unchanged()
        assert feed_s(half, len(ext)) == 0
        last = np.empty(len(ext) - half, dtype=np.int32)
        assert lib.mipgen_accel_reads_last_samples(h, last.ctypes.data_as(i32p), len(last) - 1) == E_INVALID
        assert lib.mipgen_accel_reads_last_samples(h, last.ctypes.data_as(i32p), len(last)) == 0 and np.array_equal(last, want[4][half:])
        reads = np.empty((ns + 1, n), dtype=np.int64); unique = np.empty((ns + 1, n), dtype=np.int64); row_pairs = np.empty(ns + 1, dtype=np.int64)
        tot, stot = capi.ReadTotals(), capi.SampleTotals()
        assert lib.mipgen_accel_reads_finish_samples(h, reads.ctypes.data_as(i64p), unique.ctypes.data_as(i64p), capi.C.byref(tot), capi.C.byref(stot), row_pairs.ctypes.data_as(i64p)) == 0
        assert np.array_equal(reads, want[0]) and np.array_equal(unique, want[1]) and np.array_equal(row_pairs, want[3])
        assert (tot.pairs, tot.assigned, stot.sample_none, stot.sample_ambiguous) == (want[2]["pairs"], want[2]["assigned"], want[2]["sample_none"], want[2]["sample_ambiguous"])
        unchanged()
        # a plain session refuses the samples calls, and completes
        p_want = R.count_reads(arms, ext, lig)
        assert lib.mipgen_accel_reads_open(h, arr, n, 5, 0, 0) == 0
        assert feed_s(0, half) == E_STATE
        assert lib.mipgen_accel_reads_finish_samples(h, None, None, None, None, None) == E_STATE
        assert lib.mipgen_accel_reads_last_samples(h, last.ctypes.data_as(i32p), len(last)) == E_STATE
        assert feed_p(0, len(ext)) == 0
        p_reads = np.empty(n, dtype=np.int64); p_unique = np.empty(n, dtype=np.int64)
        assert lib.mipgen_accel_reads_finish(h, p_reads.ctypes.data_as(i64p), p_unique.ctypes.data_as(i64p), None) == 0
        assert np.array_equal(p_reads, p_want[0]) and np.array_equal(p_unique, p_want[1])
        # every output of finish_samples may be NULL
        assert open_s(h, arr, n, 5, 0, 0, bc, ns, 0) == 0 and feed_s(0, 10) == 0
        assert lib.mipgen_accel_reads_finish_samples(h, None, None, None, None, None) == 0
        unchanged()
    finally:
        a.close()


def test_destroy_with_a_samples_session_open():
    a = _accel()
    arr = capi.probe_array([(b"ACGTACGTACGTACGTAA", b"ACGTACGTACGTACGTAA")])
    assert a.lib.mipgen_accel_reads_open_samples(a.h, arr, 1, 5, 0, 0, capi.c_strings([b"ACGTAC", b"TTTTTT"]), 2, 1) == 0
    off = np.array([0, 30], dtype=np.int64)
    ioff = np.array([0, 6], dtype=np.int64)
    i64p = capi.C.POINTER(capi.C.c_int64)
    assert a.lib.mipgen_accel_reads_feed_samples(a.h, 1, b"A" * 32, off.ctypes.data_as(i64p), b"C" * 32, off.ctypes.data_as(i64p), b"ACGTAC\0\0", ioff.ctypes.data_as(i64p)) == 0
    a.close()
    b = _accel()                                                                             # and the device is fine afterwards
    rows = table_rows("svr_2kb", "picked_mips")
    rng = np.random.default_rng(3)
    barcodes = draw_barcodes(rng, 3, 6)
    ext, lig, idx = lane(rows, barcodes, rng, 5, 0, 2000)
    check(b, arms_of(rows), ext, lig, idx, barcodes, 0)
    b.close()


def plain_session_digest(reads, unique, totals, assign):
    hsh = hashlib.sha256()
    for a, t in ((reads, np.int64), (unique, np.int64), (assign, np.int32)):
        hsh.update(np.ascontiguousarray(a, dtype=t).tobytes())
    hsh.update(json.dumps(totals, sort_keys=True).encode())
    return hsh.hexdigest()


def clean_reads_uneven_depth_inputs(name, key):
    """The inputs of test_gpu_reads.py::test_clean_reads_uneven_depth, drawn the same way."""
    rows = table_rows(name, key)
    rng = np.random.default_rng(11)
    ext, lig = [], []
    depth = rng.integers(0, 300, len(rows)) * (rng.random(len(rows)) > 0.25)
    if len(rows) == 1:
        depth[:] = 57
    for r, d in zip(rows, depth):
        for _ in range(int(d)):
            e, l = read_pair(r, rng, 5, 0)
            ext.append(e); lig.append(l)
    order = rng.permutation(len(ext))
    return rows, [ext[i] for i in order], [lig[i] for i in order]


@pytest.mark.parametrize("name,key", TABLES)
def test_plain_session_is_bit_identical_to_the_recorded_one(acc, name, key):
    """k_read_assign without rows: the outputs of a plain session on the inputs of test_clean_reads_uneven_depth, as SHA-256 over reads, unique_tags,
    the assignment of every pair and the totals, equal the digest recorded from the build before the samples (tests/golden/reads_plain_sessions.json)."""
    rows, ext, lig = clean_reads_uneven_depth_inputs(name, key)
    got = acc.count_reads(arms_of(rows), ext, lig, want_assignment=True)
    recorded = json.load(open(GOLDEN_PLAIN))
    assert plain_session_digest(*got) == recorded[f"{name}/{key}"]["sha256"] and len(ext) == recorded[f"{name}/{key}"]["pairs"]


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------
def _run(argv, cwd):
    return subprocess.run(argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("two_files", [False, True])
def test_cli_equals_the_oracle(tmp_path, two_files, swap):
    """-o, -samples, -labels and both stderr lines byte for byte, with one index file and with two; and without -barcodes the command writes what it
    always wrote."""
    meta = H.load_design("svr_small")
    table, rows = _subset_table(meta, "all_mips", str(tmp_path), 23)
    rng = np.random.default_rng(53 + two_files)
    J = 16 if two_files else 8
    barcodes = draw_barcodes(rng, 24, J)
    labels = [f"sample_{k:02d}" for k in range(len(barcodes))]
    ext, lig, idx = lane(rows, barcodes, rng, 5, 3, 12000, index_errors=0.05, tags_per_probe=4)
    ext = [b"N" + e[1:] if rng.random() < 0.02 else e for e in ext]
    write_fastq(tmp_path / ("lig.fq" if swap else "ext.fq"), ext)
    write_fastq(tmp_path / ("ext.fq" if swap else "lig.fq"), lig)
    with open(tmp_path / "samples.tsv", "wb") as fh:
        fh.write(b"\n".join(l.encode() + b"\t" + b for l, b in zip(labels, barcodes)) + b"\n\n")
    if two_files:
        # the second index read of some pairs is too short: no sample, whatever the first says
        i1 = [i[:10] for i in idx]
        i2 = [i[8:] if k % 50 else i[8:13] for k, i in enumerate(idx)]
        idx = [a[:8] + b[:8] if len(a) >= 8 and len(b) >= 8 else b"" for a, b in zip(i1, i2)]
        write_fastq(tmp_path / "i1.fq", i1); write_fastq(tmp_path / "i2.fq", i2)
        index_args = ["-index_reads", "i1.fq,i2.fq", "-index_length", "8,8"]
    else:
        write_fastq(tmp_path / "i1.fq", idx)
        index_args = ["-index_reads", "i1.fq"]
    common = [COUNT_BIN, "-tag_sizes", "5,3", "-mismatches", "1", "-reads", "ext.fq", "lig.fq", table] + (["-swap_reads"] if swap else [])
    p = _run(common + ["-o", "counts.tsv", "-samples", "samples_out.tsv", "-labels", "labels.tsv", "-barcodes", "samples.tsv", "-barcode_mismatches", "1"] + index_args, str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    reads, unique, tot, row_pairs, _, _ = SR.count_reads_samples(arms_of(rows), ext, lig, idx, barcodes, 1, (5, 3), 1)
    keys_names = [(r[0].decode(), r[19].decode()) for r in rows]
    assert open(tmp_path / "counts.tsv", "rb").read() == SR.counts_tsv(labels, keys_names, reads, unique)
    assert open(tmp_path / "samples_out.tsv", "rb").read() == SR.samples_tsv(labels, barcodes, reads, unique, row_pairs)
    assert open(tmp_path / "labels.tsv").read() == "".join(f"{k}\t{v}\n" for (k, _), v in zip(keys_names, SR.labels_values("tags", reads, unique)))
    assert p.stderr.decode() == SR.stderr_lines(tot, len(barcodes))
    assert tot["assigned"] > 5000 and tot["tag_n"] > 0 and tot["sample_none"] > 0 and (not two_files or tot["sample_none"] >= len(idx) // 50)
    for kind in ("reads", "log10tags"):
        q = _run(common + ["-o", "c2.tsv", "-labels", "l2.tsv", "-label", kind, "-barcodes", "samples.tsv", "-barcode_mismatches", "1"] + index_args, str(tmp_path))
        assert q.returncode == 0, q.stderr.decode()
        vals = [l.split("\t")[1] for l in open(tmp_path / "l2.tsv").read().split("\n")[:-1]]
        want = SR.labels_values(kind, reads, unique)
        assert [int(v) for v in vals] == want if kind == "reads" else [float(v) for v in vals] == want
    # without -barcodes: the lines of DESIGN 4.9, over the whole lane
    q = _run(common + ["-o", "plain.tsv"], str(tmp_path))
    assert q.returncode == 0, q.stderr.decode()
    p_reads, p_unique, p_tot, _ = R.count_reads(arms_of(rows), ext, lig, (5, 3), 1)
    assert open(tmp_path / "plain.tsv", "rb").read() == R.counts_tsv(keys_names, p_reads, p_unique)
    assert q.stderr.decode() == SR.stderr_lines(dict(p_tot, sample_none=0, sample_ambiguous=0), 0).split("\n")[0] + "\n"
    assert np.array_equal(reads.sum(axis=0), p_reads)
