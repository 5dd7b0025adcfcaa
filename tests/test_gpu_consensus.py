"""GPU: one consensus read pair per molecule (mipgen_accel_reads_open_consensus / _feed_consensus / _finish_consensus / _consensus_fetch, `mipgen_count
-consensus`).  Every case is held, by exact equality, against tests/consensus_ref.py - groups as Python dicts, votes as plain loops over
members and positions: the group list (cell, tag, family), both sequences and both quality strings - and its counts, totals and per-pair assignments
against a plain or samples session of the device on the same pairs.  Probes are a few dozen rows of the committed golden MIP tables."""
import faulthandler
import json
import os
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi, synth
from tests import consensus_ref as CR
from tests import helpers as H
from tests import reads_ref as R
from tests.test_gpu_reads import BASES, TABLES, _accel, _subset_table, arms_of, molecule, random_tag, table_rows
from tests.test_gpu_samples import GOLDEN_PLAIN, clean_reads_uneven_depth_inputs, draw_barcodes, plain_session_digest

pytestmark = pytest.mark.gpu
COUNT_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_count")
E_INVALID, E_NOMEM, E_STATE = -1, -5, -6
WG = 256                                      # CONSENSUS_WG_FAMILY (reads_common.h): above it a family is voted by a workgroup
LENGTHS = (63, 64, 65, 100, 129)              # read lengths behind the tag: below, at and above one round of 64 positions, and two rounds + 1


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


def distinct_probes(rows):
    """The rows whose own molecule is assigned to them and to nothing else: tiled probes share arm prefixes, and a read of one is a tie between two."""
    while True:
        ext = [molecule(r)[:100] for r in rows]
        lig = [R.revcomp(molecule(r))[:100] for r in rows]
        own = R.assign_reads(arms_of(rows), ext, lig, (0, 0), 0)
        keep = [r for k, r in enumerate(rows) if own[k] == k]
        if len(keep) == len(rows):
            return rows
        rows = keep


@pytest.fixture(scope="module")
def rows():
    rows = distinct_probes(table_rows("svr_small", "all_mips", 240)[::3])
    assert len(rows) >= 24
    return rows


def test_the_threshold_is_the_kernels():
    text = open(os.path.join(os.path.dirname(capi.LIB_PATH), "csrc", "reads_common.h")).read()
    assert f"#define CONSENSUS_WG_FAMILY {WG} " in text


# ---- making families -------------------------------------------------------------------------------------------------------------------------------
def qualities(rng, n, low=False):
    """n quality bytes: mostly 35..74, some '!' (0), some '~' (93); low: also bytes below 33 and above 126 (an API caller can pass them, a FASTQ line cannot)."""
    q = rng.integers(35, 75, n).astype(np.uint8)
    u = rng.random(n)
    q[u < 0.04] = ord("!"); q[(u >= 0.04) & (u < 0.07)] = ord("~")
    if low:
        q[(u >= 0.07) & (u < 0.09)] = rng.integers(0, 33, int(((u >= 0.07) & (u < 0.09)).sum()))
        q[(u >= 0.09) & (u < 0.10)] = 200
    return q.tobytes()


def member(r, rng, tag, te, n_e, n_l, err=0.04, low=False):
    """One read pair of the molecule of row r under `tag`: n_e / n_l bases behind the tags (the molecule, then random bases), sequencing errors behind the
    arms - substitutions, N and lower case - and random qualities.  The arms stay exact, so the pair is assigned at mismatches 0."""
    M = molecule(r)
    out = []
    for seq, arm, n in ((M, len(r[6]), n_e), (R.revcomp(M), len(r[10]), n_l)):
        s = bytearray((seq + random_tag(rng, max(n - len(seq), 0)))[:n])
        for j in np.flatnonzero(rng.random(n) < err):
            if j >= arm:
                s[j] = [BASES[rng.integers(0, 4)], ord("N"), s[j] | 0x20][int(rng.integers(0, 3))] if rng.random() < 0.5 else BASES[rng.integers(0, 4)]
        out.append(bytes(s))
    e, l = tag[:te] + out[0], tag[te:] + out[1]
    return e, l, qualities(rng, len(e), low), qualities(rng, len(l), low)


def families(rows, rng, sizes, te, tl, lengths=LENGTHS, low=True):
    """A family of each size, on the probes of `rows` in turn, each with a tag of its own and a read length of `lengths` in turn; shuffled."""
    pairs = []
    for k, f in enumerate(sizes):
        tag = random_tag(rng, te + tl)
        n = lengths[k % len(lengths)]
        pairs += [member(rows[k % len(rows)], rng, tag, te, n, lengths[(k + 2) % len(lengths)], low=low) for _ in range(f)]
    order = rng.permutation(len(pairs))
    return [[pairs[i][c] for i in order] for c in range(4)]


def check(acc, arms, ext, lig, eq, lq, idx=None, barcodes=None, d=0, tag_sizes=(5, 0), mismatches=0, swap_reads=False, chunks=1, arena_bytes=0):
    """The device against the oracle, the invariants, and against a plain / samples session of the device on the same pairs."""
    want = CR.consensus_reads(arms, ext, lig, eq, lq, idx, barcodes, d, tag_sizes, mismatches, swap_reads)
    got = acc.consensus_reads(arms, ext, lig, eq, lq, idx, barcodes, d, tag_sizes, mismatches, swap_reads, chunks, arena_bytes, want_assignment=True)
    reads, unique, tot, row_pairs, groups, sample, probe = got
    assert np.array_equal(probe, want[6]) and (sample is None) == (barcodes is None) and (sample is None or np.array_equal(sample, want[5]))
    assert np.array_equal(reads, want[0]) and np.array_equal(unique, want[1]) and tot == want[2]
    assert (row_pairs is None and want[3] is None) or np.array_equal(row_pairs, want[3])
    assert [g[:3] for g in groups] == [g[:3] for g in want[4]]
    for k, (g, w) in enumerate(zip(groups, want[4])):
        assert g == w, f"group {k} (cell {g[0]}, tag {g[1]}, family {g[2]}) differs"
    # invariants
    n = len(arms)
    assert len(groups) == int(unique.sum()) and groups == sorted(groups, key=lambda g: (g[0], g[1]))
    te, tl = tag_sizes
    e_, l_ = (lig, ext) if swap_reads else (ext, lig)
    dirty = np.zeros(reads.size, dtype=np.int64)
    for i, p in enumerate(probe):
        if p >= 0 and not all(c in R.ACGT for c in e_[i][:te] + l_[i][:tl]):
            dirty[(int(sample[i]) if sample[i] >= 0 else len(barcodes)) * n + p if sample is not None else p] += 1
    fam = np.zeros(reads.size, dtype=np.int64)
    for g in groups:
        fam[g[0]] += g[2]
    assert np.array_equal(fam, reads.ravel() - dirty) and int(dirty.sum()) == tot["tag_n"]
    # the other kinds of session on the same pairs
    if barcodes is None:
        p = acc.count_reads(arms, ext, lig, tag_sizes, mismatches, swap_reads, want_assignment=True)
        assert np.array_equal(reads[0], p[0]) and np.array_equal(unique[0], p[1]) and tot == p[2] and np.array_equal(probe, p[3])
    else:
        s = acc.count_reads_samples(arms, ext, lig, idx, barcodes, d, tag_sizes, mismatches, swap_reads, want_assignment=True)
        assert np.array_equal(reads, s[0]) and np.array_equal(unique, s[1]) and tot == s[2] and np.array_equal(row_pairs, s[3])
        assert np.array_equal(sample, s[4]) and np.array_equal(probe, s[5])
    return got


# ---- family sizes and lengths -------------------------------------------------------------------------------------------------------------------------
def test_family_sizes_and_lengths(acc, rows):
    """Families of 1, 2, 3, 63, 64, 65, the threshold - 1, the threshold, the threshold + 1 and 5,000 members - one wavefront and a whole workgroup with its
    LDS combine, member loops that end in every remainder of the unroll - at read lengths of 63, 64, 65, 100 and 129 behind the tag."""
    rng = np.random.default_rng(211)
    sizes = [1, 2, 3, 63, 64, 65, WG - 1, WG, WG + 1, 5000, 1, 2, 3, 4, 5, 6, 7, WG + 2, WG + 3, WG + 4, WG + 5, WG + 6, WG + 7, 4 * WG]
    ext, lig, eq, lq = families(rows, rng, sizes, 5, 0)
    _, _, _, _, groups, _, _ = check(acc, arms_of(rows), ext, lig, eq, lq)
    assert sorted(g[2] for g in groups) == sorted(sizes)
    assert {len(g[3]) for g in groups} == set(LENGTHS) == {len(g[5]) for g in groups}
    big = [g for g in groups if g[2] == 5000][0]
    assert b"N" not in big[3][:60] and set(big[4][:60]) == {ord("I")}             # 5,000 members with 4 % errors agree on every base


def test_unequal_lengths(acc, rows):
    """The consensus of a side is as long as its shortest member behind the tag - in small and in large families, and when one member ends with its arm."""
    rng = np.random.default_rng(223)
    ext, lig, eq, lq = [], [], [], []
    want_len = []
    for k, f in enumerate([2, 5, 70, WG + 40, 3]):
        r, tag = rows[k], random_tag(rng, 7)
        le = rng.integers(40, 140, f); ll = rng.integers(40, 140, f)
        if k == 4:
            le[1], ll[2] = len(r[6]), len(r[10])                                        # a member exactly tag + arm long, on each side
        for a, b in zip(le, ll):
            m = member(r, rng, tag, 4, int(a), int(b))
            ext.append(m[0]); lig.append(m[1]); eq.append(m[2]); lq.append(m[3])
        want_len.append((int(le.min()), int(ll.min())))
    _, _, _, _, groups, _, _ = check(acc, arms_of(rows), ext, lig, eq, lq, tag_sizes=(4, 3), chunks=2)
    assert sorted((len(g[3]), len(g[5])) for g in groups) == sorted(want_len)
    assert (len(rows[4][6]), len(rows[4][10])) in [(len(g[3]), len(g[5])) for g in groups]


# ---- bases and qualities ------------------------------------------------------------------------------------------------------------------------------
def crafted(r, tag, te, columns, n_members, fill_q=30):
    """n_members pairs of row r whose extension reads carry, behind the arm, one column per entry of `columns`: a list of (base, quality byte) per member."""
    E, M = r[6], molecule(r)
    lig = tag[te:] + R.revcomp(M)[:60]
    out = []
    for m in range(n_members):
        e = tag[:te] + E + bytes(c[m][0] for c in columns)
        q = bytes([fill_q + 33]) * (te + len(E)) + bytes(c[m][1] for c in columns)
        out.append((e, lig, q, bytes([fill_q + 33]) * len(lig)))
    return out


def test_bases_and_qualities(acc, rows):
    A, C, G, T, N = b"ACGTN"
    q = lambda v: v + 33
    columns3 = [
        [(A, q(30)), (C, q(30)), (G, q(5))],        # the three-way case: N (the reference's running best base would say G)
        [(A, q(21)), (C, q(20)), (N, q(40))],       # v = 1
        [(A, q(22)), (C, q(20)), (N, q(40))],       # v = 2
        [(A, q(30)), (A, q(10)), (N, q(40))],       # v = 40
        [(A, q(30)), (A, q(11)), (ord("a"), q(40))],  # v = 41
        [(N, q(40)), (T, q(9)), (T, q(9))],         # N in one member
        [(N, q(40)), (N, q(40)), (N, q(40))],       # N in all
        [(ord("g"), q(40)), (ord("t"), q(40)), (ord("c"), q(40))],   # lower case in all
        [(A, ord("!")), (C, ord("!")), (G, ord("!"))],   # no weight anywhere
        [(A, ord("~")), (C, q(60)), (C, q(20))],    # '~' is 93: A by 13
        [(A, 10), (A, 32), (G, q(3))],              # quality bytes below 33 weigh nothing
        [(A, 200), (C, q(60)), (N, 255)],           # and one above 126 weighs 93
        [(A, q(30)), (C, q(29)), (G, q(29))],       # the largest sum is below the others together
    ]
    pairs = crafted(rows[0], b"ACGTAC", 5, columns3, 3)
    # quality '!' everywhere: every position is N
    pairs += [(e, l, b"!" * len(e), b"!" * len(l)) for e, l, _, _ in crafted(rows[1], b"TTGCAA", 5, columns3, 3)]
    # the same columns over a family of the workgroup kernel: the three voters among WG + 10 members of no weight
    silent = [[c[0], c[1], c[2]] + [(T, ord("!"))] * (WG + 7) for c in columns3]
    pairs += crafted(rows[2], b"GGATCC", 5, silent, WG + 10, fill_q=0)
    ext, lig, eq, lq = ([p[c] for p in pairs] for c in range(4))
    _, _, _, _, groups, _, _ = check(acc, arms_of(rows), ext, lig, eq, lq, tag_sizes=(5, 1))
    by_probe = {g[0]: g for g in groups}
    n_arm = len(rows[0][6])
    assert by_probe[0][3][n_arm:] == b"NAAAATNNNAGAA" and by_probe[0][4][n_arm:] == b"##" + bytes([q(2)]) + b"II" + bytes([q(18)]) + b"###" + bytes([q(13), q(3), q(33)]) + b"#"
    assert by_probe[0][4][:n_arm] == b"I" * n_arm
    assert set(by_probe[1][3]) == {ord("N")} and set(by_probe[1][4]) == set(by_probe[1][6]) == {ord("#")} and set(by_probe[1][5]) == {ord("N")}
    n_arm2 = len(rows[2][6])
    assert by_probe[2][2] == WG + 10 and by_probe[2][3][n_arm2:] == by_probe[0][3][n_arm:] and by_probe[2][4][n_arm2:] == by_probe[0][4][n_arm:]
    assert set(by_probe[2][3][:n_arm2]) == {ord("N")}


# ---- tags and groups ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_sizes", [(5, 0), (4, 3), (8, 8), (0, 6)])
@pytest.mark.parametrize("swap", [False, True])
def test_tags_and_groups(acc, rows, tag_sizes, swap):
    """A dirty tag is counted and forms no group; the same tag on two probes is two groups, and so is the same tag in two samples."""
    te, tl = tag_sizes
    rng = np.random.default_rng(229 + te)
    barcodes = draw_barcodes(rng, 3, 8)
    shared = random_tag(rng, te + tl)
    pairs, idx = [], []
    for k, r in enumerate(rows[:12]):
        for tag in [shared] + [random_tag(rng, te + tl) for _ in range(int(rng.integers(1, 4)))]:
            for s in (0, 1, 1, 2, 0)[:int(rng.integers(2, 6))]:
                pairs.append(member(r, rng, tag, te, 80, 70)); idx.append(barcodes[s] if rng.random() < 0.9 else random_tag(rng, 8))
        dirty = bytearray(shared); dirty[int(rng.integers(0, te + tl))] = ord("N") if k % 2 else ord("a")
        pairs.append(member(r, rng, bytes(dirty), te, 80, 70)); idx.append(barcodes[0])
    pairs.append((b"GATTACA" * 9, b"TGTAATC" * 9, b"I" * 63, b"I" * 63)); idx.append(barcodes[1])          # an unassigned pair
    ext, lig, eq, lq = ([p[c] for p in pairs] for c in range(4))
    if swap:
        ext, lig, eq, lq = lig, ext, lq, eq
    plain = check(acc, arms_of(rows), ext, lig, eq, lq, tag_sizes=tag_sizes, swap_reads=swap)
    code = CR.tag_code(shared)
    assert sum(1 for g in plain[4] if g[1] == code) == 12 and plain[2]["tag_n"] == 12 and plain[2]["unassigned"] == 1
    if not swap:
        by_sample = check(acc, arms_of(rows), ext, lig, eq, lq, idx, barcodes, 0, tag_sizes)
        assert sum(1 for g in by_sample[4] if g[1] == code) > 24 and len(by_sample[4]) > len(plain[4])
        assert {g[0] // len(rows) for g in by_sample[4]} == {0, 1, 2, 3}


# ---- chunks and indices ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [0, 1])
def test_chunks_do_not_change_the_result(acc, rows, d):
    """1, 3 and 17 feed calls - families split across chunk boundaries - with index reads that carry substitutions."""
    rng = np.random.default_rng(233 + d)
    barcodes = draw_barcodes(rng, 5, 8)
    ext, lig, eq, lq = families(rows, rng, [1, 2, 3, 9, 40, 64, 130, WG + 30, 17, 5, 1, 1, 2, 700], 3, 2, lengths=(70, 100, 65), low=False)
    idx = []
    for _ in ext:
        i = barcodes[int(rng.integers(0, 2))]
        u = rng.random()
        if u < 0.1:
            p = int(rng.integers(0, 8))
            i = i[:p] + bytes([BASES[(list(b"ACGT").index(i[p]) + 1) & 3]]) + i[p + 1:]
        elif u < 0.15:
            i = i[:3] + b"N" + i[4:]
        idx.append(i)
    first = check(acc, arms_of(rows), ext, lig, eq, lq, idx, barcodes, d, (3, 2))
    assert first[2]["sample_none"] > 0 if d == 0 else first[2]["sample_none"] == 0
    for chunks in (3, 17):
        got = acc.consensus_reads(arms_of(rows), ext, lig, eq, lq, idx, barcodes, d, (3, 2), chunks=chunks, want_assignment=True)
        assert got[4] == first[4] and got[2] == first[2] and all(np.array_equal(a, b) for a, b in zip(got[:2] + got[3:4] + got[5:], first[:2] + first[3:4] + first[5:])), chunks
    plain = check(acc, arms_of(rows), ext, lig, eq, lq, tag_sizes=(3, 2))
    for chunks in (3, 17):
        got = acc.consensus_reads(arms_of(rows), ext, lig, eq, lq, tag_sizes=(3, 2), chunks=chunks)
        assert got[4] == plain[4] and got[2] == plain[2] and np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]), chunks


# ---- arena, refusals, state ----------------------------------------------------------------------------------------------------------------------------
def test_arena_refusals_state_and_untouched_handle(rows):
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

        arms = arms_of(rows)
        rng = np.random.default_rng(239)
        ext, lig, eq, lq = families(rows, rng, [1, 2, 3, 30, 70, WG + 20, 4, 4], 5, 0, lengths=(80, 100), low=False)
        n_pairs, half = len(ext), len(ext) // 2
        lib, h = a.lib, a.h
        i64p, i32p = capi.C.POINTER(capi.C.c_int64), capi.C.POINTER(capi.C.c_int32)
        arr, n = capi.probe_array(arms), len(arms)
        bcs = [b"ACGTACGT", b"TTGCAAGC"]
        bc = capi.c_strings(bcs)
        (eb, eo), (lb, lo), (qe, _), (ql, _) = capi.pack_reads(ext), capi.pack_reads(lig), capi.pack_reads(eq), capi.pack_reads(lq)
        idx = [bcs[k % 2] for k in range(n_pairs)]
        ib, io = capi.pack_reads(idx)
        open_c, fin_c, fetch = lib.mipgen_accel_reads_open_consensus, lib.mipgen_accel_reads_finish_consensus, lib.mipgen_accel_reads_consensus_fetch
        feed_c = lambda x, y, index=False: lib.mipgen_accel_reads_feed_consensus(
            h, y - x, eb[eo[x]:].ctypes.data, qe[eo[x]:].ctypes.data, eo[x:y + 1].ctypes.data_as(i64p), lb[lo[x]:].ctypes.data, ql[lo[x]:].ctypes.data,
            lo[x:y + 1].ctypes.data_as(i64p), ib[io[x]:].ctypes.data if index else None, io[x:y + 1].ctypes.data_as(i64p) if index else None)
        feed_p = lambda x, y: lib.mipgen_accel_reads_feed(h, y - x, eb[eo[x]:].ctypes.data, eo[x:y + 1].ctypes.data_as(i64p), lb[lo[x]:].ctypes.data, lo[x:y + 1].ctypes.data_as(i64p))
        feed_s = lambda x, y: lib.mipgen_accel_reads_feed_samples(h, y - x, eb[eo[x]:].ctypes.data, eo[x:y + 1].ctypes.data_as(i64p), lb[lo[x]:].ctypes.data,
                                                                  lo[x:y + 1].ctypes.data_as(i64p), ib[io[x]:].ctypes.data, io[x:y + 1].ctypes.data_as(i64p))
        sizes = capi.ConsensusSizes()
        # nothing is open, nothing is held
        assert feed_c(0, 1) == E_STATE and fin_c(h, None, None, None, None, None, None) == E_STATE
        assert fetch(h, None, None, None, None, None, None, None, None, None) == E_STATE; unchanged()
        # every refusal of the other opens, and the four of this one
        assert open_c(h, None, n, 5, 0, 0, None, 0, 0, 0) == E_INVALID and open_c(h, arr, 0, 5, 0, 0, None, 0, 0, 0) == E_INVALID
        assert open_c(h, arr, n, 9, 8, 0, None, 0, 0, 0) == E_INVALID and open_c(h, arr, n, -1, 3, 0, None, 0, 0, 0) == E_INVALID
        assert open_c(h, arr, n, 5, 0, 3, None, 0, 0, 0) == E_INVALID
        assert open_c(h, capi.probe_array([(b"ACGTACGTACG", b"ACGTACGTACGTACGTAA")]), 1, 5, 0, 0, None, 0, 0, 0) == E_INVALID and b"12" in lib.mipgen_accel_last_error()
        assert open_c(h, capi.probe_array([(b"ACGTACGTACGTACGTAA", None)]), 1, 5, 0, 0, None, 0, 0, 0) == E_INVALID
        assert open_c(h, arr, n, 5, 0, 0, bc, 2, 2, 0) == E_INVALID and open_c(h, arr, n, 5, 0, 0, capi.c_strings([b"ACGTACGT", b"ACGTACG"]), 2, 0, 0) == E_INVALID
        assert open_c(h, arr, n, 5, 0, 0, capi.c_strings([b"ACGTACGN"]), 1, 0, 0) == E_INVALID and open_c(h, arr, n, 5, 0, 0, capi.c_strings([b"ACGT", b"ACGT"]), 2, 0, 0) == E_INVALID
        assert open_c(h, arr, n, 0, 0, 0, None, 0, 0, 0) == E_INVALID and b"no molecules" in lib.mipgen_accel_last_error()
        assert open_c(h, arr, n, 5, 0, 0, None, 0, 0, -1) == E_INVALID and b"arena_bytes" in lib.mipgen_accel_last_error()
        assert open_c(h, arr, n, 5, 0, 0, bc, 0, 0, 0) == E_INVALID and open_c(h, arr, n, 5, 0, 0, None, 2, 0, 0) == E_INVALID; unchanged()
        # a small arena: the second chunk does not fit, the session stays as it was, and finish gives the first chunk alone
        first_bytes = 2 * (int(eo[half]) + int(lo[half])) + 44 * half + 48
        assert open_c(h, arr, n, 5, 0, 0, None, 0, 0, first_bytes + 64) == 0
        assert open_c(h, arr, n, 5, 0, 0, None, 0, 0, 0) == E_STATE and lib.mipgen_accel_reads_open(h, arr, n, 5, 0, 0) == E_STATE
        assert feed_c(0, half) == 0
        assert feed_c(half, n_pairs) == E_NOMEM and b"arena" in lib.mipgen_accel_last_error()
        assert feed_c(half, n_pairs) == E_NOMEM
        last = np.empty(half, dtype=np.int32)
        want = CR.consensus_reads(arms, ext[:half], lig[:half], eq[:half], lq[:half])
        assert lib.mipgen_accel_reads_last_assignment(h, last.ctypes.data_as(i32p), half) == 0 and np.array_equal(last, want[6])
        reads = np.empty(n, dtype=np.int64); unique = np.empty(n, dtype=np.int64)
        tot = capi.ReadTotals()
        assert fin_c(h, reads.ctypes.data_as(i64p), unique.ctypes.data_as(i64p), capi.C.byref(tot), None, None, capi.C.byref(sizes)) == 0
        assert np.array_equal(reads, want[0][0]) and np.array_equal(unique, want[1][0]) and tot.pairs == half and sizes.n_groups == len(want[4])
        assert a.consensus_fetch(sizes) == want[4]
        assert a.consensus_fetch(sizes) == want[4]                                                    # the results stay: a second fetch gives the same
        assert fetch(h, None, None, None, None, None, None, None, None, None) == 0; unchanged()
        # the wrong kind: refused, the session left as it was, and it completes correctly
        whole = CR.consensus_reads(arms, ext, lig, eq, lq)
        assert open_c(h, arr, n, 5, 0, 0, None, 0, 0, 0) == 0
        assert fetch(h, None, None, None, None, None, None, None, None, None) == E_STATE           # the open dropped the earlier results
        assert feed_c(0, half) == 0
        assert feed_p(half, n_pairs) == E_STATE and feed_s(half, n_pairs) == E_STATE
        assert lib.mipgen_accel_reads_finish(h, None, None, None) == E_STATE and lib.mipgen_accel_reads_finish_samples(h, None, None, None, None, None) == E_STATE
        assert lib.mipgen_accel_reads_last_samples(h, last.ctypes.data_as(i32p), half) == E_STATE
        assert lib.mipgen_accel_reads_feed_consensus(h, 1, eb.ctypes.data, None, eo[:2].ctypes.data_as(i64p), lb.ctypes.data, ql.ctypes.data, lo[:2].ctypes.data_as(i64p),
                                                     None, None) == E_INVALID
        bad = np.array([0, 5, 3], dtype=np.int64)
        assert lib.mipgen_accel_reads_feed_consensus(h, 2, eb.ctypes.data, qe.ctypes.data, bad.ctypes.data_as(i64p), lb.ctypes.data, ql.ctypes.data, lo[:3].ctypes.data_as(i64p),
                                                     None, None) == E_INVALID; unchanged()
        assert fetch(h, None, None, None, None, None, None, None, None, None) == E_STATE           # before the finish
        assert feed_c(half, n_pairs) == 0
        assert fin_c(h, reads.ctypes.data_as(i64p), unique.ctypes.data_as(i64p), capi.C.byref(tot), None, None, capi.C.byref(sizes)) == 0
        assert np.array_equal(reads, whole[0][0]) and np.array_equal(unique, whole[1][0]) and tot.pairs == n_pairs and a.consensus_fetch(sizes) == whole[4]
        unchanged()
        # a consensus session with samples wants the index reads; sessions of the other kinds refuse the consensus calls, complete, and leave the results held
        assert open_c(h, arr, n, 5, 0, 0, bc, 2, 1, 0) == 0
        assert feed_c(0, half) == E_INVALID and feed_c(0, n_pairs, index=True) == 0
        assert fin_c(h, None, None, None, None, None, capi.C.byref(sizes)) == 0
        with_samples = CR.consensus_reads(arms, ext, lig, eq, lq, idx, bcs, 1)
        assert a.consensus_fetch(sizes) == with_samples[4]
        assert lib.mipgen_accel_reads_open(h, arr, n, 5, 0, 0) == 0
        assert fetch(h, None, None, None, None, None, None, None, None, None) == E_STATE
        assert feed_c(0, half) == E_STATE and fin_c(h, None, None, None, None, None, None) == E_STATE
        assert feed_p(0, n_pairs) == 0
        assert lib.mipgen_accel_reads_finish(h, reads.ctypes.data_as(i64p), unique.ctypes.data_as(i64p), None) == 0
        assert np.array_equal(reads, whole[0][0]) and np.array_equal(unique, whole[1][0])
        assert lib.mipgen_accel_reads_open_samples(h, arr, n, 5, 0, 0, bc, 2, 0) == 0
        assert feed_c(0, half, index=True) == E_STATE and fin_c(h, None, None, None, None, None, None) == E_STATE
        assert lib.mipgen_accel_reads_finish_samples(h, None, None, None, None, None) == 0
        # no pair in any group: no groups, and a fetch that says so
        assert open_c(h, arr, n, 5, 0, 0, None, 0, 0, 0) == 0
        junk = np.array([0, 40], dtype=np.int64)
        assert lib.mipgen_accel_reads_feed_consensus(h, 1, b"GATTACA" * 6, b"I" * 42, junk.ctypes.data_as(i64p), b"TGTAATC" * 6, b"I" * 42, junk.ctypes.data_as(i64p), None, None) == 0
        assert fin_c(h, None, None, None, None, None, capi.C.byref(sizes)) == 0 and (sizes.n_groups, sizes.ext_bytes, sizes.lig_bytes) == (0, 0, 0)
        assert a.consensus_fetch(sizes) == []
        unchanged()
    finally:
        a.close()


def test_destroy_with_a_consensus_session_open_and_with_results_held(rows):
    rng = np.random.default_rng(241)
    ext, lig, eq, lq = families(rows, rng, [3, 70, WG + 5], 5, 0, lengths=(80,), low=False)
    a = _accel()
    a.consensus_reads(arms_of(rows), ext, lig, eq, lq)                                               # results held ...
    arr = capi.probe_array(arms_of(rows))
    assert a.lib.mipgen_accel_reads_open_consensus(a.h, arr, len(rows), 5, 0, 0, None, 0, 0, 0) == 0  # ... dropped, and a session open with a chunk retained
    (eb, eo), (lb, lo), (qe, _), (ql, _) = capi.pack_reads(ext), capi.pack_reads(lig), capi.pack_reads(eq), capi.pack_reads(lq)
    i64p = capi.C.POINTER(capi.C.c_int64)
    assert a.lib.mipgen_accel_reads_feed_consensus(a.h, len(ext), eb.ctypes.data, qe.ctypes.data, eo.ctypes.data_as(i64p), lb.ctypes.data, ql.ctypes.data, lo.ctypes.data_as(i64p),
                                                   None, None) == 0
    a.close()
    b = _accel()
    check(b, arms_of(rows), ext, lig, eq, lq)
    b.close()                                                                                        # results held at destroy


@pytest.mark.parametrize("name,key", TABLES[:2])
def test_a_plain_session_afterwards_is_the_recorded_one(acc, rows, name, key):
    rng = np.random.default_rng(251)
    ext, lig, eq, lq = families(rows, rng, [2, 66], 5, 0, lengths=(70,), low=False)
    acc.consensus_reads(arms_of(rows), ext, lig, eq, lq)
    t_rows, t_ext, t_lig = clean_reads_uneven_depth_inputs(name, key)
    got = acc.count_reads(arms_of(t_rows), t_ext, t_lig, want_assignment=True)
    recorded = json.load(open(GOLDEN_PLAIN))
    assert plain_session_digest(*got) == recorded[f"{name}/{key}"]["sha256"]


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------
def write_fastq_q(path, reads, quals):
    with open(path, "wb") as fh:
        for i, (r, q) in enumerate(zip(reads, quals)):
            fh.write(b"@r%d\n" % i + r + b"\n+\n" + q + b"\n")


def _run(argv, cwd):
    return subprocess.run(argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


@pytest.mark.parametrize("with_barcodes", [False, True])
def test_cli_equals_the_oracle(tmp_path, with_barcodes):
    """Both FASTQ files byte for byte and the stderr line, with and without -barcodes, at -min_family 1 and 2; -o is what it is without -consensus."""
    meta = H.load_design("svr_small")
    table, t_rows = _subset_table(meta, "all_mips", str(tmp_path), 23)
    own = R.assign_reads(arms_of(t_rows), [molecule(r)[:100] for r in t_rows], [R.revcomp(molecule(r))[:100] for r in t_rows], (0, 0), 0)
    t_rows_used = [r for k, r in enumerate(t_rows) if own[k] == k][:40]                              # probes whose own molecule is no tie within the table
    assert len(t_rows_used) == 40
    rng = np.random.default_rng(257 + with_barcodes)
    sizes = [1] * 30 + [2, 2, 3, 5, 8, 64, 65, WG + 9, 1, 1]
    ext, lig, eq, lq = families(t_rows_used, rng, sizes, 5, 3, lengths=(90, 100, 75), low=False)
    ext[7] = b"N" + ext[7][1:]                                                                       # a dirty tag
    barcodes = draw_barcodes(rng, 4, 8)
    labels = [f"sample_{k}" for k in range(4)]
    idx = [barcodes[int(rng.integers(0, 3))] if rng.random() < 0.95 else random_tag(rng, 8) for _ in ext]
    write_fastq_q(tmp_path / "ext.fq", ext, eq); write_fastq_q(tmp_path / "lig.fq", lig, lq)
    write_fastq_q(tmp_path / "i1.fq", idx, [b"I" * 8] * len(idx))
    with open(tmp_path / "samples.tsv", "wb") as fh:
        fh.write(b"\n".join(l.encode() + b"\t" + b for l, b in zip(labels, barcodes)) + b"\n")
    common = [COUNT_BIN, "-tag_sizes", "5,3", "-reads", "ext.fq", "lig.fq", table] + (["-barcodes", "samples.tsv", "-index_reads", "i1.fq"] if with_barcodes else [])
    want = CR.consensus_reads(arms_of(t_rows), ext, lig, eq, lq, idx if with_barcodes else None, barcodes if with_barcodes else None, 0, (5, 3))
    keys = [r[0].decode() for r in t_rows]
    base = _run(common + ["-o", "plain.tsv"], str(tmp_path))
    assert base.returncode == 0, base.stderr.decode()
    for k in (1, 2):
        p = _run(common + ["-o", "counts.tsv", "-consensus", f"smc{k}"] + (["-min_family", "2"] if k == 2 else []), str(tmp_path))
        assert p.returncode == 0, p.stderr.decode()
        e, l, line = CR.consensus_fastq(want[4], keys, 8, labels if with_barcodes else None, k)
        assert open(tmp_path / f"smc{k}.ext.fq", "rb").read() == e and open(tmp_path / f"smc{k}.lig.fq", "rb").read() == l
        assert p.stderr.decode() == base.stderr.decode() + line
        assert open(tmp_path / "counts.tsv", "rb").read() == open(tmp_path / "plain.tsv", "rb").read()
    assert e.count(b"@smc") == sum(1 for g in want[4] if g[2] >= 2) >= 7 and want[2]["tag_n"] == 1
