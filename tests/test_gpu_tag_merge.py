"""GPU: molecular tags one substitution apart merged by the count rule before the consensus (mipgen_accel_reads_set_tag_mismatches / _last_tag_merge /
_tag_map_fetch, `mipgen_count -tag_mismatches 1 -tag_map`).  Every case is held, by exact equality, against tests/tag_merge_ref.py - raw groups as
Python dicts, every pair of tags of a cell compared by plain loops: the corrected group list (cell, tag, family), both consensus sequences and quality strings,
the raw-to-corrected map and the totals - and its reads, totals and per-pair assignments against the same session at tag mismatches 0."""
import faulthandler
import json
import os

import numpy as np
import pytest

from mipgen_amd import capi
from tests import consensus_ref as CR
from tests import helpers as H
from tests import pileup_ref as PR
from tests import reads_ref as R
from tests import tag_merge_ref as TM
from tests.test_gpu_consensus import WG, _run, crafted, distinct_probes, member, write_fastq_q
from tests.test_gpu_reads import _accel, _subset_table, arms_of, molecule, random_tag, table_rows
from tests.test_gpu_samples import GOLDEN_PLAIN, clean_reads_uneven_depth_inputs, draw_barcodes, plain_session_digest

pytestmark = pytest.mark.gpu
COUNT_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_count")
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
def rows():
    rows = distinct_probes(table_rows("svr_small", "all_mips", 240)[::3])
    assert len(rows) >= 24
    return rows


def sub(tag: bytes, at: int, step: int = 1) -> bytes:
    """`tag` with the base at `at` replaced by the one `step` (1..3) further along A C G T."""
    return tag[:at] + bytes([b"ACGT"[(b"ACGT".index(tag[at]) + step) & 3]]) + tag[at + 1:]


def family(r, rng, tag, te, count, n_e=60, n_l=50, err=0.03):
    """`count` read pairs of the molecule of row r under `tag`, with sequencing errors behind the arms."""
    return [member(r, rng, tag, te, n_e, n_l, err=err, low=False) for _ in range(count)]


def check(acc, arms, pairs, idx=None, barcodes=None, tag_sizes=(5, 0), chunks=1, shuffle=None):
    """The device at tag mismatches 1 against the oracle - groups, map, totals -, the invariants, and the same session at tag mismatches 0."""
    if shuffle is not None:
        order = shuffle.permutation(len(pairs))
        pairs = [pairs[i] for i in order]
        idx = None if idx is None else [idx[i] for i in order]
    ext, lig, eq, lq = ([p[c] for p in pairs] for c in range(4))
    want = TM.consensus_reads(arms, ext, lig, eq, lq, idx, barcodes, 0, tag_sizes, 0, 1)
    got = acc.consensus_reads(arms, ext, lig, eq, lq, idx, barcodes, 0, tag_sizes, chunks=chunks, want_assignment=True, tag_mismatches=1)
    totals, tag_map = acc.last_tag_merge(), acc.tag_map_fetch()
    reads, unique, tot, row_pairs, groups, sample, probe = got
    assert [g[:3] for g in groups] == [g[:3] for g in want[4]]
    for k, (g, w) in enumerate(zip(groups, want[4])):
        assert g == w, f"group {k} (cell {g[0]}, tag {g[1]}, family {g[2]}) differs"
    assert tag_map == want[7]
    assert totals == want[8]
    assert np.array_equal(reads, want[0]) and np.array_equal(unique, want[1]) and tot == want[2] and np.array_equal(probe, want[6])
    # the invariants, against the session with the merge off
    off = acc.consensus_reads(arms, ext, lig, eq, lq, idx, barcodes, 0, tag_sizes, chunks=chunks, want_assignment=True)
    assert np.array_equal(reads, off[0]) and tot == off[2] and np.array_equal(probe, off[6])
    assert (row_pairs is None and off[3] is None) or np.array_equal(row_pairs, off[3])
    assert (sample is None and off[5] is None) or np.array_equal(sample, off[5])
    assert len(groups) == int(unique.sum()) == totals["groups"] and len(off[4]) == totals["raw_groups"]
    assert sum(g[2] for g in groups) == sum(g[2] for g in off[4])
    assert totals["raw_groups"] - totals["groups"] == totals["absorbed"]
    assert [(m[0], m[1], m[2]) for m in tag_map] == [g[:3] for g in off[4]]
    return groups, tag_map, totals, off


# ---- the thresholds of the rule ------------------------------------------------------------------------------------------------------------------------
def test_rule_thresholds(acc, rows):
    """One cell (probe) per hand-written case: 1 + 1, 2 + 1, 3 + 2, 2 + 2, 10 + 6, 11 + 6, the larger of two eligible parents, equal counts, the chain X100 - Y5 - Z1."""
    rng = np.random.default_rng(3001)
    X = b"ACGTA"
    cases = [[(X, 1), (sub(X, 4), 1)], [(X, 2), (sub(X, 4), 1)], [(X, 3), (sub(X, 0), 2)], [(X, 2), (sub(X, 2), 2)], [(X, 10), (sub(X, 1), 6)], [(X, 11), (sub(X, 1), 6)],
             [(X, 1), (sub(X, 4), 5), (sub(X, 0), 7)], [(X, 1), (sub(X, 4, 3), 5), (sub(X, 4, 1), 5)], [(X, 1), (sub(X, 0, 3), 5), (sub(X, 4, 2), 5)],
             [(X, 100), (sub(X, 4), 5), (sub(sub(X, 4), 3), 1)]]
    pairs = []
    for k, case in enumerate(cases):
        for tag, count in case:
            pairs += family(rows[k], rng, tag, 5, count)
    groups, tag_map, totals, _ = check(acc, arms_of(rows), pairs, shuffle=rng)
    c = lambda t: CR.tag_code(t)
    by_cell = lambda k: [(m[1], m[3]) for m in tag_map if m[0] == k]
    assert [len({m[3] for m in tag_map if m[0] == k}) for k in range(10)] == [2, 1, 1, 2, 2, 1, 2, 2, 2, 1]
    assert dict(by_cell(6))[c(X)] == c(sub(X, 0)) and dict(by_cell(7))[c(X)] == c(sub(X, 4, 1)) and dict(by_cell(8))[c(X)] == c(sub(X, 4, 2))
    assert set(dict(by_cell(9)).values()) == {c(X)} and totals["max_depth"] == 2
    assert [g[2] for g in groups if g[0] == 9] == [106]


# ---- lanes ---------------------------------------------------------------------------------------------------------------------------------------------
def test_lanes(acc, rows):
    """Cells of 1, 63, 64, 65 and 257 raw tags; a hub of 40 with all 15 singleton neighbours; a hub's neighbour that is itself a parent; the chain of depth 6."""
    rng = np.random.default_rng(3011)
    pairs = []
    for k, n_tags in enumerate((1, 63, 64, 65, 257)):
        codes = rng.choice(1024, n_tags, replace=False)
        for code in codes:
            tag = CR.tag_string(int(code), 5).encode()
            pairs += family(rows[k], rng, tag, 5, int(rng.choice([1, 1, 1, 2, 3, 5])), n_e=40, n_l=36)
    hub = b"GATCC"
    pairs += family(rows[5], rng, hub, 5, 40)
    for at in range(5):
        for step in (1, 2, 3):
            pairs += family(rows[5], rng, sub(hub, at, step), 5, 1)
    pairs += family(rows[6], rng, hub, 5, 40) + family(rows[6], rng, sub(hub, 2), 5, 3) + family(rows[6], rng, sub(sub(hub, 2), 0), 5, 1)
    chain = [b"AAAAA", b"AAAAC", b"AAACC", b"AACCC", b"ACCCC", b"CCCCC", b"CCCCG"]
    for tag, count in zip(chain, (33, 17, 9, 5, 3, 2, 1)):
        pairs += family(rows[7], rng, tag, 5, count, n_e=40, n_l=36)
    groups, tag_map, totals, _ = check(acc, arms_of(rows), pairs, shuffle=rng)
    assert totals["max_depth"] == 6
    assert [g[1:3] for g in groups if g[0] == 5] == [(CR.tag_code(hub), 55)] and [g[1:3] for g in groups if g[0] == 6] == [(CR.tag_code(hub), 44)]
    assert [g[1:3] for g in groups if g[0] == 7] == [(0, 70)]
    assert [sum(1 for m in tag_map if m[0] == k) for k in range(5)] == [1, 63, 64, 65, 257]


# ---- cell boundaries -----------------------------------------------------------------------------------------------------------------------------------
def test_cell_boundaries(acc, rows):
    rng = np.random.default_rng(3023)
    barcodes = draw_barcodes(rng, 2, 8)
    X, Y = b"CAGTA", b"CAGTC"
    pairs, idx = [], []

    def add(r, tag, count, s):
        fam = family(rows[r], rng, tag, 5, count)
        pairs.extend(fam); idx.extend([barcodes[s]] * len(fam))
    # the same two neighbouring tags on two probes and in two samples: four groups stay four
    add(0, X, 5, 0); add(1, Y, 1, 0); add(0, Y, 1, 1); add(1, X, 5, 1)
    # a tag whose only neighbour lies in the next cell; the last code of a cell beside the first of the next
    add(3, b"TTTTT", 1, 0); add(4, b"TTTTG", 9, 0); add(4, b"AAAAA", 9, 0); add(5, b"AAAAC", 1, 0)
    add(len(rows) - 1, b"TTTTT", 1, 0); add(0, b"AAAAA", 9, 1); add(0, b"TTTTA", 9, 1)        # ... across the sample rows too
    groups, tag_map, totals, _ = check(acc, arms_of(rows), pairs, idx, barcodes, shuffle=rng)
    assert totals["absorbed"] == 0 and totals["groups"] == 11 and all(m[1] == m[3] for m in tag_map)
    # and within one cell the same tags do merge
    pairs2 = family(rows[0], rng, X, 5, 5) + family(rows[0], rng, Y, 5, 1)
    _, _, totals2, _ = check(acc, arms_of(rows), pairs2, [barcodes[0]] * 6, barcodes)
    assert totals2 == {"raw_groups": 2, "groups": 1, "absorbed": 1, "moved_pairs": 1, "max_depth": 1}


# ---- tag shapes ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag_sizes", [(5, 0), (1, 0), (0, 6), (8, 8), (4, 3)])
def test_tag_shapes(acc, rows, tag_sizes):
    """A substitution at the first and at the last tag base, in the extension part and in the ligation part; a dirty tag one base from a clean one joins nothing."""
    te, tl = tag_sizes
    T = te + tl
    rng = np.random.default_rng(3037 + T)
    pairs = []
    spots = sorted({0, T - 1, max(te - 1, 0), min(te, T - 1)})
    for k, at in enumerate(spots):
        tag = random_tag(rng, T) if T < 16 else b"T" + random_tag(rng, 15)                # (8,8: the top bit of the code set)
        pairs += family(rows[k], rng, tag, te, 6) + family(rows[k], rng, sub(tag, at, 1 + k % 3), te, 1)
    clean = random_tag(rng, T)
    dirty = clean[:T - 1] + b"N"
    pairs += family(rows[6], rng, clean, te, 4) + family(rows[6], rng, dirty, te, 1)
    groups, tag_map, totals, off = check(acc, arms_of(rows), pairs, tag_sizes=tag_sizes, shuffle=rng)
    assert totals["absorbed"] == len(spots) and totals["moved_pairs"] == len(spots) and totals["groups"] == len(spots) + 1
    assert [g[2] for g in groups] == [7] * len(spots) + [4]


# ---- the vote sees the absorbed members -----------------------------------------------------------------------------------------------------------------
def test_vote_paths(acc, rows):
    """200 + 57 merge to 257 and go through the workgroup kernel, 250 + 5 stay on the one-wavefront kernel; a position where only the merged sums flip the base."""
    rng = np.random.default_rng(3041)
    X = b"GGCATA"
    pairs = family(rows[0], rng, X, 5, 200, err=0.01) + family(rows[0], rng, sub(X, 2), 5, 57, err=0.01)
    pairs += family(rows[1], rng, X, 5, 250, err=0.01) + family(rows[1], rng, sub(X, 0), 5, 5, err=0.01)
    A, C = b"AC"
    pairs += crafted(rows[2], X, 5, [[(A, 20 + 33), (A, 20 + 33)]], 2) + crafted(rows[2], sub(X, 5), 5, [[(C, 60 + 33)]], 1)
    groups, _, totals, off = check(acc, arms_of(rows), pairs, tag_sizes=(5, 1), shuffle=rng)
    assert [g[2] for g in groups] == [257, 255, 3] and WG == 256 and totals["absorbed"] == 3
    n_arm = len(rows[2][6])
    alone = [g for g in off[4] if g[0] == 2 and g[2] == 2][0]
    assert alone[3][n_arm:] == b"A" and groups[2][3][n_arm:] == b"C" and groups[2][4][n_arm:] == bytes([20 + 33])


# ---- chunks --------------------------------------------------------------------------------------------------------------------------------------------
def test_chunks_do_not_change_the_result(acc, rows):
    rng = np.random.default_rng(3049)
    pairs = []
    for k in range(12):
        tag = random_tag(rng, 7)
        pairs += family(rows[k], rng, tag, 4, int(rng.choice([2, 5, 30, 70])))
        for _ in range(int(rng.integers(1, 4))):
            pairs += family(rows[k], rng, sub(tag, int(rng.integers(0, 7)), int(rng.integers(1, 4))), 4, int(rng.choice([1, 1, 2])))
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]                                                    # families and their erroneous copies split across the chunks
    results = [check(acc, arms_of(rows), pairs, tag_sizes=(4, 3), chunks=c)[:3] for c in (1, 3, 17)]
    assert results[0] == results[1] == results[2] and results[0][2]["absorbed"] >= 12


# ---- off means off -------------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(acc, rows):
    rng = np.random.default_rng(3061)
    X = b"TGCAA"
    pairs = family(rows[0], rng, X, 5, 9) + family(rows[0], rng, sub(X, 1), 5, 1) + family(rows[1], rng, X, 5, 2)
    ext, lig, eq, lq = ([p[c] for p in pairs] for c in range(4))
    arms = arms_of(rows)
    want = CR.consensus_reads(arms, ext, lig, eq, lq)
    never = acc.consensus_reads(arms, ext, lig, eq, lq, want_assignment=True)
    t_never, m_never = acc.last_tag_merge(), acc.tag_map_fetch()
    explicit = acc.consensus_reads(arms, ext, lig, eq, lq, want_assignment=True, after_open=lambda: acc.set_tag_mismatches(0))
    t_explicit, m_explicit = acc.last_tag_merge(), acc.tag_map_fetch()
    back = acc.consensus_reads(arms, ext, lig, eq, lq, want_assignment=True, after_open=lambda: (acc.set_tag_mismatches(1), acc.set_tag_mismatches(0)))
    for got in (never, explicit, back):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[4] == want[4] and np.array_equal(got[6], want[6])
    assert t_never == t_explicit == acc.last_tag_merge() == {"raw_groups": 3, "groups": 3, "absorbed": 0, "moved_pairs": 0, "max_depth": 0}
    assert m_never == m_explicit == acc.tag_map_fetch() == [(g[0], g[1], g[2], g[1]) for g in want[4]]
    # a new open resets the setting: the session after a merging one does not merge
    assert acc.consensus_reads(arms, ext, lig, eq, lq, tag_mismatches=1)[4] != want[4]
    assert acc.consensus_reads(arms, ext, lig, eq, lq)[4] == want[4]


@pytest.mark.parametrize("name,key", [("svr_small", "all_mips")])
def test_a_plain_session_afterwards_is_the_recorded_one(acc, rows, name, key):
    rng = np.random.default_rng(3067)
    pairs = family(rows[0], rng, b"ACCGT", 5, 9) + family(rows[0], rng, b"ACCGA", 5, 1)
    ext, lig, eq, lq = ([p[c] for p in pairs] for c in range(4))
    acc.consensus_reads(arms_of(rows), ext, lig, eq, lq, tag_mismatches=1)
    assert acc.last_tag_merge()["absorbed"] == 1
    t_rows, t_ext, t_lig = clean_reads_uneven_depth_inputs(name, key)
    got = acc.count_reads(arms_of(t_rows), t_ext, t_lig, want_assignment=True)
    assert plain_session_digest(*got) == json.load(open(GOLDEN_PLAIN))[f"{name}/{key}"]["sha256"]


# ---- downstream ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_pileup_loses_the_false_molecule(acc, rows):
    """30 molecules of one probe; one of them also appears as a single read with a tag error and a base substitution: depth 31 and a false allele without the
    merge, depth 30 and none with it - both equal to pileup_ref over the oracle's groups."""
    rng = np.random.default_rng(3079)
    r = rows[0]
    M = molecule(r)
    tags = set()
    while len(tags) < 30:
        t = random_tag(rng, 8)
        if all(sum(a != b for a, b in zip(t, u)) > 2 for u in tags):                      # (no two true molecules within two bases of each other)
            tags.add(t)
    tags = sorted(tags)
    pairs = []
    for t in tags:
        pairs += family(r, rng, t, 8, 4, n_e=80, n_l=70, err=0.0)
    at = len(r[6]) + 7                                                                    # a target base behind the extension arm
    assert 8 + at < 88 and len(M) - 1 - at >= 70                                          # the extension reads cover it, the ligation reads do not
    wrong = b"ACGT"[(b"ACGT".index(M[at]) + 1) & 3]
    e, l, qe, ql = family(r, rng, sub(tags[11], 3), 8, 1, n_e=80, n_l=70, err=0.0)[0]
    pairs.append((e[:8 + at] + bytes([wrong]) + e[8 + at + 1:], l, qe, ql))
    ext, lig, eq, lq = ([p[c] for p in pairs] for c in range(4))
    arms, n = arms_of(rows), len(rows)
    mol_len = [len(molecule(x)) for x in rows]
    col = b"ACGT".index(wrong)
    for d, depth, false_allele in ((0, 31, 1), (1, 30, 0)):
        want = TM.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=(8, 0), tag_mismatches=d)
        acc.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=(8, 0), tag_mismatches=d)
        counts, totals = acc.consensus_pileup(mol_len, 0, 1, 0)
        w_counts, w_totals = PR.pileup(want[4], mol_len, n, 0, 1, 0)
        assert np.array_equal(counts, w_counts) and totals == w_totals
        assert int(counts[at, :4].sum()) == depth and int(counts[at, col]) == false_allele and totals["used"] == depth


# ---- state and refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_state_and_refusals(rows):
    rng = np.random.default_rng(3083)
    from mipgen_amd import synth
    genome = synth.random_genome(12000, 5)
    P = capi.make_params(130, 140, score_method=capi.SCORE_LOGISTIC, arm_pairs=synth.arm_pairs_from_sums([43, 44]))
    a = capi.Accel(P)
    try:
        a.upload([capi.build_region(genome, "1", 5000, 5055, P, bwa_mode="hashed", label="s1")])
        a.score_resident(capi.SCORE_LOGISTIC)
        s0, r0 = a.download()
        lib, h = a.lib, a.h
        C = capi.C
        tot = capi.TagMergeTotals()
        setter, last, fetch = lib.mipgen_accel_reads_set_tag_mismatches, lib.mipgen_accel_reads_last_tag_merge, lib.mipgen_accel_reads_tag_map_fetch
        assert setter(h, 1) == E_STATE and b"no read-counting session" in lib.mipgen_accel_last_error()
        assert last(h, C.byref(tot)) == E_STATE and fetch(h, None, None, None, None) == E_STATE
        pairs = family(rows[0], rng, b"ACCGT", 5, 9) + family(rows[0], rng, b"ACCGA", 5, 1)
        ext, lig, eq, lq = ([p[c] for p in pairs] for c in range(4))
        arms = arms_of(rows)
        barcodes = draw_barcodes(rng, 2, 8)
        idx = [barcodes[0]] * len(ext)

        def refused():
            assert setter(h, 1) == E_STATE and b"keeps no reads" in lib.mipgen_accel_last_error()
        plain = a._read_session(arms, ext, lig, after_open=refused)                       # the session completes afterwards
        assert int(plain[0].sum()) == 10 and int(plain[1].sum()) == 2
        smp = a._read_session(arms, ext, lig, None, idx, barcodes, after_open=refused)
        assert int(smp[0].sum()) == 10 and int(smp[1].sum()) == 2

        def bad_values():
            assert setter(h, 2) == E_INVALID and setter(h, -1) == E_INVALID and b"outside 0..1" in lib.mipgen_accel_last_error()
            assert last(h, C.byref(tot)) == E_STATE and fetch(h, None, None, None, None) == E_STATE      # before the finish
            assert setter(h, 1) == 0
        got = a.consensus_reads(arms, ext, lig, eq, lq, after_open=bad_values)
        assert [g[2] for g in got[4]] == [10] and a.last_tag_merge()["absorbed"] == 1
        assert fetch(h, None, None, None, None) == 0 and last(h, None) == E_INVALID
        arr = capi.probe_array(arms)
        assert lib.mipgen_accel_reads_open_consensus(h, arr, len(rows), 5, 0, 0, None, 0, 0, 0) == 0
        assert last(h, C.byref(tot)) == E_STATE and fetch(h, None, None, None, None) == E_STATE          # after the next open
        assert lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, None) == 0
        assert last(h, C.byref(tot)) == 0 and (tot.raw_groups, tot.groups, tot.absorbed) == (0, 0, 0) and a.tag_map_fetch() == []
        s1, r1 = a.download()                                                             # the dense results of the handle are unchanged
        assert np.array_equal(s1.view(np.int64), s0.view(np.int64)) and np.array_equal(r1, r0)
        a.consensus_reads(arms, ext, lig, eq, lq, tag_mismatches=1)                       # destroy with the map held
    finally:
        a.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_barcodes", [False, True])
def test_cli_equals_the_oracle(tmp_path, with_barcodes):
    """-tag_mismatches 1 -tag_map with and without -barcodes, with and without -consensus: the map, the counts and the FASTQ files byte for byte against files
    written from the oracle, and the stderr line; -tag_mismatches 0 is byte-identical to no option."""
    meta = H.load_design("svr_small")
    table, t_rows = _subset_table(meta, "all_mips", str(tmp_path), 23)
    own = R.assign_reads(arms_of(t_rows), [molecule(r)[:100] for r in t_rows], [R.revcomp(molecule(r))[:100] for r in t_rows], (0, 0), 0)
    used = [r for k, r in enumerate(t_rows) if own[k] == k][:12]
    rng = np.random.default_rng(3089 + with_barcodes)
    barcodes = draw_barcodes(rng, 3, 8)
    labels = [f"sample_{k}" for k in range(3)]
    pairs, idx = [], []
    for k, r in enumerate(used):
        tag = random_tag(rng, 8)
        s = int(rng.integers(0, 3))
        fam = family(r, rng, tag, 5, int(rng.choice([3, 8, 20])), n_e=80, n_l=70) + family(r, rng, sub(tag, int(rng.integers(0, 8))), 5, 1 + k % 2, n_e=80, n_l=70)
        fam += family(r, rng, random_tag(rng, 8), 5, 1, n_e=80, n_l=70)
        pairs += fam; idx += [barcodes[s] if rng.random() < 0.95 else random_tag(rng, 8) for _ in fam]
    order = rng.permutation(len(pairs))
    pairs, idx = [pairs[i] for i in order], [idx[i] for i in order]
    ext, lig, eq, lq = ([p[c] for p in pairs] for c in range(4))
    to_fastq = lambda q: bytes(min(max(b, 33), 126) for b in q)
    eq, lq = [to_fastq(q) for q in eq], [to_fastq(q) for q in lq]
    write_fastq_q(tmp_path / "ext.fq", ext, eq); write_fastq_q(tmp_path / "lig.fq", lig, lq)
    write_fastq_q(tmp_path / "i1.fq", idx, [b"I" * 8] * len(idx))
    with open(tmp_path / "samples.tsv", "wb") as fh:
        fh.write(b"\n".join(l.encode() + b"\t" + b for l, b in zip(labels, barcodes)) + b"\n")
    common = [COUNT_BIN, "-tag_sizes", "5,3", "-reads", "ext.fq", "lig.fq", table] + (["-barcodes", "samples.tsv", "-index_reads", "i1.fq"] if with_barcodes else [])
    want = TM.consensus_reads(arms_of(t_rows), ext, lig, eq, lq, idx if with_barcodes else None, barcodes if with_barcodes else None, 0, (5, 3), 0, 1)
    assert want[8]["absorbed"] >= 8
    keys = [r[0].decode() for r in t_rows]
    lab = labels if with_barcodes else None
    # off: no option, and the option at 0
    base = _run(common + ["-o", "plain.tsv", "-consensus", "off"], str(tmp_path))
    zero = _run(common + ["-o", "zero.tsv", "-consensus", "zero", "-tag_mismatches", "0"], str(tmp_path))
    assert base.returncode == 0 and zero.returncode == 0, base.stderr.decode() + zero.stderr.decode()
    assert zero.stderr == base.stderr and b"tag_mismatches" not in base.stderr
    for a, b in (("plain.tsv", "zero.tsv"), ("off.ext.fq", "zero.ext.fq"), ("off.lig.fq", "zero.lig.fq")):
        assert open(tmp_path / a, "rb").read() == open(tmp_path / b, "rb").read()
    # on, without -consensus: the counts and the map
    p = _run(common + ["-o", "counts.tsv", "-tag_mismatches", "1", "-tag_map", "map.tsv"], str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert open(tmp_path / "map.tsv", "rb").read() == TM.tag_map_file(want[7], keys, 8, lab)
    first = base.stderr.decode().split("mipgen_count: consensus")[0]
    assert p.stderr.decode() == first + TM.stderr_line(want[8])
    counts = open(tmp_path / "counts.tsv").read().splitlines()[1:]
    got_unique = {tuple(l.split("\t")[:1 + with_barcodes]): int(l.split("\t")[-1]) for l in counts}      # (sample,) mip_key -> unique_tags
    want_unique = {(((labels[row] if row < 3 else "undetermined"), keys[pr]) if with_barcodes else (keys[pr],)): int(u)
                   for (row, pr), u in np.ndenumerate(want[1]) if want[0][row, pr] > 0 or not with_barcodes}
    assert got_unique == want_unique and sum(want_unique.values()) == want[8]["groups"]
    # on, with -consensus: the FASTQ files carry the corrected tag and the merged family
    q = _run(common + ["-o", "counts2.tsv", "-consensus", "on", "-tag_mismatches", "1", "-tag_map", "map2.tsv"], str(tmp_path))
    assert q.returncode == 0, q.stderr.decode()
    e, l, line = CR.consensus_fastq(want[4], keys, 8, lab, 1)
    assert open(tmp_path / "on.ext.fq", "rb").read() == e and open(tmp_path / "on.lig.fq", "rb").read() == l
    assert q.stderr.decode() == first + line + TM.stderr_line(want[8])
    assert open(tmp_path / "map2.tsv", "rb").read() == open(tmp_path / "map.tsv", "rb").read()
    assert open(tmp_path / "counts2.tsv", "rb").read() == open(tmp_path / "counts.tsv", "rb").read()
