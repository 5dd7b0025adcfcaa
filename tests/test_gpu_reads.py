"""GPU: reads and unique tags per probe from smMIP read pairs (mipgen_accel_reads_open / _feed / _finish, `mipgen_count`).  Every case is
held, by exact equality, against tests/reads_ref.py - the capture model restated by brute force, every pair against every probe.  Probes are rows
of the committed golden MIP tables (both strands); the read pairs are made from M = E + T + L by a seeded generator."""
import faulthandler
import math
import os
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi, synth
from tests import helpers as H
from tests import reads_ref as R
from tests.probe_tables import golden_table, rescore_argv

pytestmark = pytest.mark.gpu
BIN_DIR = os.path.dirname(capi.LIB_PATH)
COUNT_BIN = os.path.join(BIN_DIR, "mipgen_count")
TRAIN_BIN = os.path.join(BIN_DIR, "mipgen_svr_train")
TABLES = [("svr_small", "all_mips"), ("svr_2kb", "picked_mips"), ("long_capture_svr", "picked_mips"), ("logistic_snp_trf", "all_mips")]
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def table_rows(name, key, limit=320):
    """Rows (lists of byte fields) of a golden table: a run of neighbouring rows (tiled probes share arms) and a spread over the rest."""
    lines = H.ref_lines(H.load_design(name), key)[1:]
    rows = [l.split(b"\t") for l in lines]
    if len(rows) > limit:
        rows = rows[:limit // 2] + rows[limit // 2::max(1, (len(rows) - limit // 2) // (limit // 2))][:limit // 2]
    return rows


def arms_of(rows):
    return [(r[6], r[10]) for r in rows]


def molecule(r):
    return r[6] + r[13] + r[10]                                 # M = E + T + L


def random_tag(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes()


def read_pair(r, rng, te, tl, read_len=100, tag=None):
    """The two reads of a molecule captured by the probe of row r: tag_e + M ..., tag_l + revcomp(M) ..."""
    M = molecule(r)
    tag = random_tag(rng, te + tl) if tag is None else tag
    return tag[:te] + M[:read_len - te], tag[te:] + R.revcomp(M)[:read_len - tl]


def substitute(read, pos, rng):
    """Another of A C G T at `pos`."""
    c = read[pos:pos + 1]
    return read[:pos] + bytes([rng.choice([b for b in b"ACGT" if bytes([b]) != c])]) + read[pos + 1:]


def _accel():
    return capi.Accel(capi.make_params(152, 162, score_method=capi.SCORE_LOGISTIC))


def check(acc, arms, ext, lig, tag_sizes=(5, 0), mismatches=0, swap_reads=False, chunks=1, key_buffer=0):
    """The device against the oracle: reads, unique_tags, totals and the assignment of every pair."""
    w_reads, w_unique, w_tot, w_assign = R.count_reads(arms, ext, lig, tag_sizes, mismatches, swap_reads)
    reads, unique, tot, assign = acc.count_reads(arms, ext, lig, tag_sizes, mismatches, swap_reads, chunks, key_buffer, want_assignment=True)
    assert np.array_equal(assign, w_assign), f"first pair that differs: {int(np.flatnonzero(assign != w_assign)[0])}"
    assert np.array_equal(reads, w_reads) and np.array_equal(unique, w_unique)
    assert tot == w_tot, (tot, w_tot)
    return reads, unique, tot, assign


@pytest.fixture(scope="module")
def acc():
    a = _accel()
    yield a
    a.close()


@pytest.mark.parametrize("name,key", TABLES)
def test_clean_reads_uneven_depth(acc, name, key):
    """Clean reads of every table, both strands, with a depth per probe between zero and a few hundred."""
    rows = table_rows(name, key)
    assert len({r[17] for r in rows}) == 2 or len(rows) == 1
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
    ext, lig = [ext[i] for i in order], [lig[i] for i in order]
    reads, unique, tot, _ = check(acc, arms_of(rows), ext, lig)
    assert tot["pairs"] == len(ext) and tot["assigned"] + tot["ambiguous"] + tot["unassigned"] == len(ext) and tot["assigned"] > 0
    assert (reads == 0).any() or len(rows) == 1


@pytest.mark.parametrize("tag_sizes", [(5, 0), (4, 3), (0, 0), (8, 8), (0, 6)])
def test_tag_duplicates(acc, tag_sizes):
    """PCR families: a few tags per probe, each read several times; the same tag on two probes counts for both."""
    te, tl = tag_sizes
    rows = table_rows("svr_small", "all_mips", 120)[::3]
    rng = np.random.default_rng(5)
    shared = [random_tag(rng, te + tl) for _ in range(3)]
    ext, lig = [], []
    for k, r in enumerate(rows):
        tags = shared + [random_tag(rng, te + tl) for _ in range(int(rng.integers(0, 6)))]
        for t in tags:
            for _ in range(int(rng.integers(1, 9))):
                e, l = read_pair(r, rng, te, tl, tag=t)
                ext.append(e); lig.append(l)
    reads, unique, tot, assign = check(acc, arms_of(rows), ext, lig, tag_sizes)
    if te + tl == 0:
        assert np.array_equal(unique, reads)
    else:
        assigned = np.flatnonzero(reads)
        assert len(assigned) > 10 and (unique[assigned] >= 3).all() and (unique[assigned] < reads[assigned]).any()


@pytest.mark.parametrize("m", [0, 1, 2])
def test_substitutions(acc, m):
    """Substitutions in the seed, beyond the seed, in one arm and in both, at every allowed mismatch count.  A pair whose extension seed is broken is
    still found through its ligation seed, and the reverse; with both seeds broken it is unassigned whatever m is."""
    rows = [r for r in table_rows("svr_small", "all_mips", 200)[::2] if min(len(r[6]), len(r[10])) > 16]
    arms = arms_of(rows)
    S = R.seed_length(arms)
    rng = np.random.default_rng(17 + m)
    te, tl = 5, 2
    ext, lig, kind = [], [], []
    for p, r in enumerate(rows):
        le, ll = len(r[6]), len(r[10])
        plans = {
            "ext_seed": ([int(rng.integers(0, S))], []), "lig_seed": ([], [int(rng.integers(0, S))]),
            "ext_beyond": ([int(rng.integers(S, le))] if le > S else [le - 1], []), "lig_beyond": ([], [int(rng.integers(S, ll))] if ll > S else [ll - 1]),
            "both_seeds": ([int(rng.integers(0, S))], [int(rng.integers(0, S))]),
            "ext_two": (sorted(rng.choice(le, 2, replace=False).tolist()), []), "both_arms_beyond": ([le - 1], [ll - 1]),
            "ext_three": (sorted(rng.choice(le, 3, replace=False).tolist()), []), "insert_only": ([le + 3], [ll + 3]),
        }
        for name, (pe, pl) in plans.items():
            e, l = read_pair(r, rng, te, tl)
            for q in pe:
                e = substitute(e, te + q, rng)
            for q in pl:
                l = substitute(l, tl + q, rng)
            ext.append(e); lig.append(l); kind.append((name, p))
    _, _, _, assign = check(acc, arms, ext, lig, (te, tl), m)
    by_kind = {}
    for (name, p), a in zip(kind, assign):
        by_kind.setdefault(name, []).append((p, int(a)))
    assert all(a == R.UNASSIGNED for _, a in by_kind["both_seeds"])                         # at every m
    assert all(a >= 0 or a == R.AMBIGUOUS for _, a in by_kind["insert_only"])
    if m >= 1:
        # found through the other seed (tiled neighbours may tie: then ambiguous, never unassigned)
        assert all(a != R.UNASSIGNED for _, a in by_kind["ext_seed"]) and sum(a == p for p, a in by_kind["ext_seed"]) > len(rows) // 2
        assert all(a != R.UNASSIGNED for _, a in by_kind["lig_seed"]) and sum(a == p for p, a in by_kind["lig_seed"]) > len(rows) // 2
    else:
        assert all(a != p for p, a in by_kind["ext_seed"]) and all(a != p for p, a in by_kind["ext_beyond"])
    assert all(a != p for p, a in by_kind["ext_three"])


def test_n_and_lower_case(acc):
    """N and lower-case bytes in the arms of a read are mismatches; in a tag they keep the pair out of every tag group (tag_n)."""
    rows = table_rows("logistic_snp_trf", "all_mips", 160)[::2]
    rng = np.random.default_rng(23)
    te, tl = 5, 3
    ext, lig = [], []
    for r in rows:
        for variant in range(8):
            e, l = read_pair(r, rng, te, tl)
            if variant == 1:
                e = b"N" + e[1:]                                                             # tag
            elif variant == 2:
                l = l[:1] + l[1:2].lower() + l[2:]                                           # tag, lower case
            elif variant == 3:
                e = e[:te + 2] + b"N" + e[te + 3:]                                           # seed
            elif variant == 4:
                q = tl + len(r[10]) - 1
                l = l[:q] + l[q:q + 1].lower() + l[q + 1:]                                   # last base of the ligation arm
            elif variant == 5:
                e = e.lower()
            elif variant == 6:
                e = e[:2] + b"n" + e[3:]; l = l[:0] + b"." + l[1:]
            ext.append(e); lig.append(l)
    for m in (0, 1):
        _, _, tot, _ = check(acc, arms_of(rows), ext, lig, (te, tl), m)
        assert tot["tag_n"] > 0
    # N and lower case in a probe's own arm: that base matches nothing
    arms = arms_of(rows)
    arms[3] = (arms[3][0][:14] + b"N" + arms[3][0][15:], arms[3][1])
    arms[5] = (arms[5][0], arms[5][1][:-3] + arms[5][1][-3:].lower())
    for m in (0, 1, 2):
        check(acc, arms, ext, lig, (te, tl), m)


def test_short_and_empty_reads(acc):
    """Reads shorter than tag + arm, shorter than the tag, and empty reads fail; a read that ends with the arm's last base passes."""
    rows = table_rows("svr_small", "all_mips", 60)
    rng = np.random.default_rng(29)
    te, tl = 5, 4
    ext, lig = [], []
    for r in rows:
        e, l = read_pair(r, rng, te, tl)
        le, ll = te + len(r[6]), tl + len(r[10])
        for ce, cl in [(le, ll), (le - 1, ll), (le, ll - 1), (0, ll), (le, 0), (0, 0), (te, tl), (3, 2), (le + 1, ll + 7), (te + 12, 100), (100, tl + 12)]:
            ext.append(e[:ce]); lig.append(l[:cl])
    for m in (0, 2):
        _, _, tot, assign = check(acc, arms_of(rows), ext, lig, (te, tl), m, chunks=3)
        by_cut = assign.reshape(len(rows), 11)
        # no arm fits in a read of at most 12 bases behind its tag (the shortest arm has 16); a read cut one base short may still be a tiled
        # neighbour's whole arm, so those columns are the oracle's to say
        assert (by_cut[:, 3:8] == R.UNASSIGNED).all() and (by_cut[:, 9:] == R.UNASSIGNED).all()
        assert (by_cut[:, 0] != R.UNASSIGNED).all() and (by_cut[:, 8] != R.UNASSIGNED).all() and tot["unassigned"] >= 7 * len(rows)


def test_ambiguity(acc):
    """Two rows with identical arms always tie; a probe that differs from another by one base loses to it on an exact read (fewest mismatches) and
    ties with it on a read that misses both by one."""
    rows = [r for r in table_rows("svr_small", "all_mips", 100)[::5] if len(r[6]) >= 20]
    rng = np.random.default_rng(31)
    arms = arms_of(rows)
    n0 = len(arms)
    arms.append(arms[0])                                                                    # row n0: the arms of row 0 again
    q = len(arms[1][0]) - 2                                                                 # row n0 + 1: row 1 with one other base near the end of E (beyond the seed)
    S = R.seed_length(arms)
    assert q >= S
    arms.append((substitute(arms[1][0], q, rng), arms[1][1]))
    third = [b for b in b"ACGT" if bytes([b]) not in (arms[1][0][q:q + 1], arms[-1][0][q:q + 1])][0]
    ext, lig, what = [], [], []
    for _ in range(20):
        e, l = read_pair(rows[0], rng, 5, 0); ext.append(e); lig.append(l); what.append("dup")
        e, l = read_pair(rows[1], rng, 5, 0); ext.append(e); lig.append(l); what.append("exact1")
        ext.append(e[:5 + q] + bytes([third]) + e[5 + q + 1:]); lig.append(l); what.append("between")
        e, l = read_pair(rows[2], rng, 5, 0); ext.append(e); lig.append(l); what.append("plain")
    what = np.array(what)
    for m in (0, 1, 2):
        reads, _, tot, assign = check(acc, arms, ext, lig, (5, 0), m, chunks=2)
        assert (assign[what == "dup"] == R.AMBIGUOUS).all() and reads[0] == 0 and reads[n0] == 0
        assert (assign[what == "exact1"] == 1).all()                                        # 0 mismatches beats 1
        assert (assign[what == "plain"] == 2).all()
        assert (assign[what == "between"] == (R.AMBIGUOUS if m >= 1 else R.UNASSIGNED)).all()


def test_unrelated_reads_are_unassigned(acc):
    """Random sequence and the reads of another table's probes."""
    rows = table_rows("svr_small", "all_mips", 200)
    others = table_rows("long_capture_svr", "picked_mips") + table_rows("svr_2kb", "picked_mips")
    own = {a for a in arms_of(rows)}
    others = [r for r in others if (r[6], r[10]) not in own]
    rng = np.random.default_rng(37)
    ext, lig = [], []
    for _ in range(3000):
        ext.append(random_tag(rng, 100)); lig.append(random_tag(rng, 100))
    for r in others:
        for _ in range(40):
            e, l = read_pair(r, rng, 5, 0)
            ext.append(e); lig.append(l)
    for r in rows[::9]:
        e, l = read_pair(r, rng, 5, 0)
        ext.append(e); lig.append(l)
    _, _, tot, assign = check(acc, arms_of(rows), ext, lig, (5, 0), 2)
    assert (assign[:3000] == R.UNASSIGNED).all() and tot["unassigned"] >= 3000


def _mixed_reads(rows, rng, te, tl, depth):
    ext, lig = [], []
    for r in rows:
        tags = [random_tag(rng, te + tl) for _ in range(4)]
        for _ in range(int(rng.integers(0, depth))):
            e, l = read_pair(r, rng, te, tl, tag=tags[int(rng.integers(0, 4))] if rng.random() < 0.7 else None)
            if rng.random() < 0.1:
                e = substitute(e, int(rng.integers(0, 40)), rng)
            if rng.random() < 0.03:
                e = b"N" + e[1:]
            ext.append(e); lig.append(l)
    order = rng.permutation(len(ext))
    return [ext[i] for i in order], [lig[i] for i in order]


def test_swap_reads(acc):
    rows = table_rows("svr_small", "all_mips", 100)
    rng = np.random.default_rng(41)
    ext, lig = _mixed_reads(rows, rng, 5, 2, 30)
    a = check(acc, arms_of(rows), ext, lig, (5, 2), 1)
    b = check(acc, arms_of(rows), lig, ext, (5, 2), 1, swap_reads=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[2]["assigned"] > 0
    c = acc.count_reads(arms_of(rows), lig, ext, (5, 2), 1)                                   # the files the wrong way round: next to nothing is found
    assert c[2]["assigned"] < a[2]["assigned"] // 10


def test_chunks_and_key_buffer_do_not_change_the_result(acc):
    """The same pairs fed as 1, 3 and 17 chunks, and with a key buffer of a few hundred keys (sort-unique whenever it fills, growth when more than
    half of it is distinct keys), give identical arrays."""
    rows = table_rows("logistic_snp_trf", "all_mips", 300)
    rng = np.random.default_rng(43)
    ext, lig = _mixed_reads(rows, rng, 4, 4, 200)
    assert 20000 < len(ext) < 300000
    first = check(acc, arms_of(rows), ext, lig, (4, 4), 1)
    for chunks, key_buffer in [(3, 0), (17, 0), (1, 256), (5, 3000), (17, 1)]:
        got = acc.count_reads(arms_of(rows), ext, lig, (4, 4), 1, chunks=chunks, key_buffer=key_buffer, want_assignment=True)
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]) and got[2] == first[2] and np.array_equal(got[3], first[3]), (chunks, key_buffer)


def test_timing_does_not_change_the_result():
    """Each kind of session with the HIP-event timing off and on: every output is the same, and mipgen_accel_last_kernel_ms 7..10 hold what each
    kind leaves there.  The plain session in 3 chunks with 1,024 keys sorts or grows its key buffer between calls (a call of about 700 pairs is one k_read_assign
    launch, or two where the buffer has between 512 and 700 keys free).  "plain, one call": all pairs (> 1,800) in one feed call against a buffer of 256 keys - a launch takes no more pairs
    than the buffer has free keys, 256 at first and at most twice as many after each growth, so that one call makes several timed launches."""
    rows = table_rows("svr_small", "all_mips", limit=40)
    arms = arms_of(rows)
    rng = np.random.default_rng(61)
    ext, lig = _mixed_reads(rows, rng, 5, 0, 100)
    assert 1800 < len(ext) < 2600
    barcodes = [b"ACGTACGT", b"TTGCAAGC", b"GGATCCTA", b"CATGTGAC"]
    idx = [barcodes[int(k)] for k in rng.integers(0, 4, len(ext))]
    eq, lq = [bytes(rng.integers(35, 74, len(r), dtype=np.uint8)) for r in ext], [bytes(rng.integers(35, 74, len(r), dtype=np.uint8)) for r in lig]
    kinds = {
        "plain": lambda a: a.count_reads(arms, ext, lig, (5, 0), chunks=3, key_buffer=1024, want_assignment=True),
        "plain, one call": lambda a: a.count_reads(arms, ext, lig, (5, 0), chunks=1, key_buffer=256, want_assignment=True),
        "samples": lambda a: a.count_reads_samples(arms, ext, lig, idx, barcodes, tag_sizes=(5, 0), chunks=2, want_assignment=True),
        "consensus": lambda a: a.consensus_reads(arms, ext, lig, eq, lq, idx, barcodes, tag_sizes=(5, 0), chunks=2, want_assignment=True),
    }

    def same(x, y):
        return np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y

    a = _accel()                                                                             # (a fresh handle: 7..10 start at -1.0)
    try:
        for kind, run in kinds.items():
            plain = kind.startswith("plain")
            a.set_timing(False)
            off = run(a)
            ms_off = [a.last_kernel_ms(k) for k in (7, 8, 9, 10)]
            a.set_timing(True)
            on = run(a)
            ms_on = [a.last_kernel_ms(k) for k in (7, 8, 9, 10)]
            print(kind, ms_off, ms_on)
            assert len(off) == len(on) and all(same(x, y) for x, y in zip(off, on)), kind
            assert off[2]["assigned"] > 1000
            # timing off: every open zeroes 7, a samples open zeroes 8 and another sets it to -1.0, a consensus finish sets 9 and 10 to -1.0
            assert ms_off == [0.0, -1.0 if plain else 0.0, -1.0, -1.0], kind
            assert ms_on[0] > 0.0, kind
            assert ms_on[1] == -1.0 if plain else ms_on[1] > 0.0, kind
            assert (ms_on[2] > 0.0 and ms_on[3] > 0.0) if kind == "consensus" else ms_on[2:] == [-1.0, -1.0], kind
    finally:
        a.set_timing(False)
        a.close()


def test_handle_state_is_untouched_and_refusals(acc):
    """A dense result of the handle downloads unchanged after a session and after every refused call; refusals carry their codes."""
    genome = synth.random_genome(12000, 5)
    P = capi.make_params(130, 140, score_method=capi.SCORE_LOGISTIC, arm_pairs=synth.arm_pairs_from_sums([43, 44]))
    a = capi.Accel(P)
    try:
        regions = [capi.build_region(genome, "1", 5000, 5055, P, bwa_mode="hashed", label="s1")]
        a.upload(regions)
        a.score_resident(capi.SCORE_LOGISTIC)
        s0, r0 = a.download()

        def unchanged():
            s, r = a.download()
            assert np.array_equal(s.view(np.int64), s0.view(np.int64)) and np.array_equal(r, r0)

        rows = table_rows("svr_small", "all_mips", 80)
        rng = np.random.default_rng(47)
        ext, lig = _mixed_reads(rows, rng, 5, 0, 20)
        check(a, arms_of(rows), ext, lig)
        unchanged()
        lib, h = a.lib, a.h
        i64p = capi.C.POINTER(capi.C.c_int64)
        one = np.zeros(2, dtype=np.int64)
        arr = (capi.Probe * 2)(capi.Probe(b"ACGTACGTACGTACGT", b"ACGTACGTACGTACGTAA", None, None, 0, 0, -1, 0), capi.Probe(b"ACGTACGTACGTACGTT", b"CCGTACGTACGTACGTAA", None, None, 0, 0, -1, 0))
        E_INVALID, E_STATE = -1, -6
        assert lib.mipgen_accel_reads_feed(h, 1, b"A", one.ctypes.data_as(i64p), b"A", one.ctypes.data_as(i64p)) == E_STATE; unchanged()
        assert lib.mipgen_accel_reads_finish(h, None, None, None) == E_STATE; unchanged()
        assert lib.mipgen_accel_reads_open(h, None, 2, 5, 0, 0) == E_INVALID; unchanged()
        assert lib.mipgen_accel_reads_open(h, arr, 0, 5, 0, 0) == E_INVALID
        assert lib.mipgen_accel_reads_open(h, arr, 2, 9, 8, 0) == E_INVALID
        assert lib.mipgen_accel_reads_open(h, arr, 2, -1, 0, 0) == E_INVALID
        assert lib.mipgen_accel_reads_open(h, arr, 2, 5, 0, 3) == E_INVALID
        assert lib.mipgen_accel_reads_open(h, arr, 2, 5, 0, -1) == E_INVALID; unchanged()
        short = (capi.Probe * 1)(capi.Probe(b"ACGTACGTACG", b"ACGTACGTACGTACGTAA", None, None, 0, 0, -1, 0))
        assert lib.mipgen_accel_reads_open(h, short, 1, 5, 0, 0) == E_INVALID and b"12" in lib.mipgen_accel_last_error()
        empty = (capi.Probe * 1)(capi.Probe(b"", b"ACGTACGTACGTACGTAA", None, None, 0, 0, -1, 0))
        assert lib.mipgen_accel_reads_open(h, empty, 1, 5, 0, 0) == E_INVALID
        null = (capi.Probe * 1)(capi.Probe(b"ACGTACGTACGTACGTAA", None, None, None, 0, 0, -1, 0))
        assert lib.mipgen_accel_reads_open(h, null, 1, 5, 0, 0) == E_INVALID
        long_ = (capi.Probe * 1)(capi.Probe(b"ACGT" * 17, b"ACGTACGTACGTACGTAA", None, None, 0, 0, -1, 0))
        assert lib.mipgen_accel_reads_open(h, long_, 1, 5, 0, 0) == E_INVALID; unchanged()
        assert lib.mipgen_accel_reads_open(h, arr, 2, 5, 0, 0) == 0
        assert lib.mipgen_accel_reads_open(h, arr, 2, 5, 0, 0) == E_STATE                       # one session at a time
        bad = np.array([0, 5, 3], dtype=np.int64)
        assert lib.mipgen_accel_reads_feed(h, 2, b"AAAAAAAA", bad.ctypes.data_as(i64p), b"AAAAAAAA", bad.ctypes.data_as(i64p)) == E_INVALID
        assert lib.mipgen_accel_reads_feed(h, 1, None, one.ctypes.data_as(i64p), b"A", one.ctypes.data_as(i64p)) == E_INVALID
        unchanged()
        assert lib.mipgen_accel_reads_finish(h, None, None, None) == 0
        unchanged()
    finally:
        a.close()


def test_destroy_with_a_session_open():
    a = _accel()
    arr = (capi.Probe * 1)(capi.Probe(b"ACGTACGTACGTACGTAA", b"ACGTACGTACGTACGTAA", None, None, 0, 0, -1, 0))
    assert a.lib.mipgen_accel_reads_open(a.h, arr, 1, 5, 0, 0) == 0
    off = np.array([0, 30], dtype=np.int64)
    i64p = capi.C.POINTER(capi.C.c_int64)
    assert a.lib.mipgen_accel_reads_feed(a.h, 1, b"A" * 32, off.ctypes.data_as(i64p), b"C" * 32, off.ctypes.data_as(i64p)) == 0
    a.close()
    b = _accel()                                                                             # and the device is fine afterwards
    rows = table_rows("svr_2kb", "picked_mips")
    rng = np.random.default_rng(3)
    ext, lig = _mixed_reads(rows, rng, 5, 0, 20)
    check(b, arms_of(rows), ext, lig)
    b.close()


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def write_fastq(path, reads):
    with open(path, "wb") as fh:
        for i, r in enumerate(reads):
            fh.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def _run(argv, cwd):
    return subprocess.run(argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def _subset_table(meta, key, work, step):
    """A table of a few hundred rows of distinct probes: the header and every step-th row of a golden table."""
    src = open(golden_table(meta, key, work), "rb").read().split(b"\n")
    rows = [l for l in src[1:] if l][::step]
    path = os.path.join(work, "probes.txt")
    with open(path, "wb") as fh:
        fh.write(b"\n".join([src[0]] + rows) + b"\n")
    return path, [l.split(b"\t") for l in rows]


@pytest.mark.parametrize("swap", [False, True])
def test_cli_counts_equal_the_oracle(tmp_path, swap):
    meta = H.load_design("svr_small")
    table, rows = _subset_table(meta, "all_mips", str(tmp_path), 23)
    assert 200 < len(rows) < 400
    rng = np.random.default_rng(53)
    ext, lig = _mixed_reads(rows, rng, 5, 3, 60)
    write_fastq(tmp_path / ("lig.fq" if swap else "ext.fq"), ext)
    write_fastq(tmp_path / ("ext.fq" if swap else "lig.fq"), lig)
    argv = [COUNT_BIN, "-tag_sizes", "5,3", "-mismatches", "1", "-o", "counts.tsv", "-reads", "ext.fq", "lig.fq", table] + (["-swap_reads"] if swap else [])
    p = _run(argv, str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    reads, unique, tot, _ = R.count_reads(arms_of(rows), ext, lig, (5, 3), 1)
    want = R.counts_tsv([(r[0].decode(), r[19].decode()) for r in rows], reads, unique)
    assert open(tmp_path / "counts.tsv", "rb").read() == want
    assert p.stderr.decode() == (f"mipgen_count: pairs {tot['pairs']} assigned {tot['assigned']} ambiguous {tot['ambiguous']} unassigned {tot['unassigned']} "
                                 f"tag_n {tot['tag_n']} overflow 0\n")
    assert tot["assigned"] > 1000 and tot["tag_n"] > 0


@pytest.mark.parametrize("label", ["tags", "log10tags"])
def test_cli_count_rescore_train_loop(tmp_path, label):
    """mipgen_count -labels -> mipgen_rescore -features -labels -> mipgen_svr_train with no edit in between leaves a model."""
    meta = H.load_design("svr_small")
    table, rows = _subset_table(meta, "all_mips", str(tmp_path), 23)
    rng = np.random.default_rng(59)
    ext, lig = _mixed_reads(rows, rng, 5, 0, 80)
    write_fastq(tmp_path / "ext.fq", ext); write_fastq(tmp_path / "lig.fq", lig)
    p = _run([COUNT_BIN, "-o", "counts.tsv", "-labels", "labels.tsv", "-label", label, "-reads", "ext.fq", "lig.fq", table], str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    _, unique, _, _ = R.count_reads(arms_of(rows), ext, lig, (5, 0), 0)
    lab = [l.split("\t") for l in open(tmp_path / "labels.tsv").read().split("\n")[:-1]]
    assert [k for k, _ in lab] == [r[0].decode() for r in rows]
    if label == "tags":
        assert [int(v) for _, v in lab] == unique.tolist()
    else:
        assert [float(v) for _, v in lab] == [math.log10(u + 1.0) for u in unique.tolist()]               # (the C library's log10, as the tool calls it)
    p = _run(rescore_argv(meta, str(tmp_path)) + ["-features", "rows.libsvm", "-labels", "labels.tsv", table], str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert f"{len(rows)} training rows written, 0 probes without a label skipped" in p.stderr.decode()
    t = _run([TRAIN_BIN, "-q", "-g", "0.05", "-c", "2", "rows.libsvm", "rows.model"], str(tmp_path))
    assert t.returncode == 0, t.stderr.decode()
    assert open(tmp_path / "rows.model").read().startswith("svm_type epsilon_svr")


def test_cli_malformed_fastq_names_file_and_line(tmp_path):
    meta = H.load_design("svr_2kb")
    table = golden_table(meta, "picked_mips", str(tmp_path))
    write_fastq(tmp_path / "ext.fq", [b"ACGT" * 10] * 3)
    with open(tmp_path / "lig.fq", "wb") as fh:
        fh.write(b"@r0\nACGT\n+\nIIII\n@r1\nACGT\n+\nIII\n")
    p = _run([COUNT_BIN, "-o", "counts.tsv", "-reads", "ext.fq", "lig.fq", table], str(tmp_path))
    assert p.returncode == 1 and "lig.fq:8: malformed FASTQ record (sequence and quality differ in length)" in p.stderr.decode(), p.stderr.decode()
    assert not os.path.exists(tmp_path / "counts.tsv")
