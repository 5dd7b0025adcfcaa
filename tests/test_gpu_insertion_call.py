"""GPU: insertion alleles called against a background of the other samples, from reads (mipgen_accel_reads_consensus_insertion_pool, _insertion_pool_fetch,
_reads_consensus_insertion_call, _insertion_call_fetch, `mipgen_count -call_insertions`).  Every comparison is exact equality with
tests/insertion_call_ref.py - dictionaries and plain sums over tests/insertion_ref.py's rows - on the groups the device itself fetched.  A candidate whose exact
score lies within 1e-6 of an integer is dropped from both sides, at most 1 in 1,000 of a test's candidates."""
import faulthandler

import numpy as np
import pytest

from mipgen_amd import capi, synth
from tests import call_ref as CR
from tests import consensus_ref as CONS
from tests import gapped_ref as G
from tests import helpers as H
from tests import insertion_call_ref as IC
from tests import insertion_ref as I
from tests import reads_ref as R
from tests.test_gpu_gapped import PAD, variant
from tests.test_gpu_insertions import quiet_sites, with_insert
from tests.test_gpu_pileup import ARM, COUNT_BIN, TAGS, Lane, _run, cut_probes, session, write_fastq_q
from tests.test_gpu_reads import _accel, random_tag
from tests.test_gpu_samples import draw_barcodes
from tests.test_pileup_cpu import clean_window, synthetic_row
from tests.test_reads_cpu import HEADER

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -6
P1 = CR.params(min_depth=5, min_alt=2, min_ppm=0, min_q=0, a0=1, n0=1024, bg_max_ppm=200000)     # (n0 no power of 10: k = n under the prior alone is no integer score)


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def genome():
    return synth.random_genome(40000, 17)


def planted_lane(genome, seed):
    """Three samples and undetermined over molecules of 40, 64, 65, 129 and 70 bases, 10 plain molecules per (row, probe), and planted: a private insertion (sample
    0), a shared low-rate one (every row), a carrier above bg_max_ppm (sample 1, with one molecule each in samples 0 and 2), two alleles of one anchor, an insertion
    only the ligation read reaches, an ambiguous one, and - the template of the last probe being its sequence without base 1 and without the last but one, and its
    reads 40 bases long, so that each end is seen from its own side only - an insertion at anchors 0 and L - 2 in every molecule of that probe.  (templates, arms,
    barcodes, lane columns)."""
    rng = np.random.default_rng(seed)
    mols, arms = cut_probes(genome, [40, 64, 65, 129, 70])
    S = mols[4]
    templates = mols[:4] + [S[:1] + S[2:-2] + S[-1:]]
    barcodes = draw_barcodes(rng, 3, 8)
    index = lambda s: barcodes[s] if s < 3 else b"N" * 8
    L = Lane(rng)
    for s in range(4):
        for M in mols:
            for k in range(10):
                L.molecule(M, 40 if M is S else len(M), 40 if M is S else len(M), index=index(s), qual=ord("I"))
    both = lambda M, at, X, s, times: [variant(L, M, with_insert(M, at, X), with_insert(M, at, X), len(M) + len(X), len(M) + len(X), qual=ord("I"), index=index(s))
                                       for _ in range(times)]
    a, d = quiet_sites(mols[3], 30, 60)[0], quiet_sites(mols[3], 70, 110)[0]
    both(mols[3], a, b"GC", 0, 4)                                                                             # private
    b, e = quiet_sites(mols[1], ARM + 1, 30)[0], quiet_sites(mols[1], 34, 64 - ARM)[0]
    for s in range(4):
        both(mols[1], b, b"G", s, 1)                                                                          # shared, low rate
    c = quiet_sites(mols[2], ARM + 1, 65 - ARM)[0]
    both(mols[2], c, b"CG", 1, 8); both(mols[2], c, b"CG", 0, 1); both(mols[2], c, b"CG", 2, 1)               # a carrier at 8 of 18
    both(mols[3], d, b"GGC", 2, 3); both(mols[3], d, b"GGG", 2, 2); both(mols[3], d, b"GGC", 0, 1)            # two alleles of one anchor
    M = mols[0]
    f = quiet_sites(M, ARM + 2, 40 - ARM)[0]
    for _ in range(3):
        variant(L, M, M, with_insert(M, f, b"C"), ARM + 1, len(M) + 1, qual=ord("I"), index=index(0))        # only the ligation read reaches it
    Mv = with_insert(mols[1], e, b"GCG")
    for _ in range(2):
        variant(L, mols[1], Mv[:e + 1] + b"N" + Mv[e + 2:], Mv, len(Mv), ARM + 1, qual=ord("I"), index=index(2))   # N inside the run, the other read too short
    return templates, arms, barcodes, L.shuffled()


def compare_pool(acc, rows, n_sample, totals, bg):
    w_pool, w_S = IC.sparse_pool(rows[:n_sample], bg)
    assert totals == {"rows": n_sample, "entries": sum(len(r.count) for r in rows[:n_sample]), "alleles": len(w_pool)}, totals
    pool, S = acc.insertion_pool_fetch(totals["alleles"])
    assert pool.dtype == capi.INSERTION_POOL_RECORD_DTYPE and pool.tobytes() == w_pool.tobytes() and np.array_equal(S, w_S)
    return w_pool


def compare_call(acc, row, want, p, budget):
    """One insertion call of `row`, twice, against the oracle's (totals, candidates); what it returns."""
    params = capi.CallParams(**p)
    res = acc.consensus_insertion_call(row, params)
    again = acc.consensus_insertion_call(row, params)
    assert all(x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y for x, y in zip(res, again))
    counts, anchors, it, recs, ct = res
    w_totals, cands = want
    assert {k: ct[k] for k in ("tested", "too_deep", "candidates")} == {k: w_totals[k] for k in ("tested", "too_deep", "candidates")}, (row, ct, w_totals)
    assert IC.drop_excluded(recs, cands) == IC.kept_calls(cands, p), (row, recs, cands)
    assert w_totals["calls"] <= ct["calls"] <= w_totals["calls"] + w_totals["excluded"] and not recs["reserved"].any()
    budget[0] += w_totals["candidates"]; budget[1] += w_totals["excluded"]
    return res


@pytest.mark.parametrize("W", [4, 15])
def test_pool_and_calls_of_a_planted_lane(genome, W):
    templates, arms, barcodes, cols = planted_lane(genome, 811)
    lens = [len(t) for t in templates]
    a = _accel()
    try:
        got, want = session(a, arms, cols, barcodes)
        assert got == want
        rows = IC.session_rows(got, templates, 4, 1, 0, W)
        plain = [a.consensus_insertions(templates, lens, r, 1, 0, W) for r in range(4)]
        budget = [0, 0]
        for p in (P1, dict(P1, min_q=25, bg_max_ppm=500000)):
            totals = a.consensus_insertion_pool(templates, lens, 1, 0, W, p["bg_max_ppm"])
            with pytest.raises(RuntimeError):
                a.insertions_fetch(0)                                                                         # (the pool's last row is no insertions call)
            w_pool = compare_pool(a, rows, 3, totals, p["bg_max_ppm"])
            runs = {sum(1 for r in rows[:3] if (int(q["pos"]), int(q["length"]), int(q["bases"])) in r.count) for q in w_pool}
            assert runs == {1, 2, 3}                                                                          # alleles of one, two and all sample rows
            if p is P1:
                assert (w_pool["bg_excluded"] > 0).any() and (w_pool["bg_excluded"] == 0).any()                 # the carrier of probe 2; the last probe's everywhere
            oracle = IC.call_session(rows, True, p)
            for r in (2, 0, 3, 1, 0):
                counts, anchors, it, recs, ct = compare_call(a, r, oracle[r], p, budget)
                assert counts.tobytes() == plain[r][0].tobytes() and anchors.tobytes() == plain[r][1].tobytes() and it == plain[r][3]
                assert a.insertions_fetch(it["alleles"]).tobytes() == plain[r][2].tobytes()
            with pytest.raises(RuntimeError, match="bg_max_ppm"):
                a.consensus_insertion_call(0, capi.CallParams(**dict(p, bg_max_ppm=p["bg_max_ppm"] + 1)))
        assert budget[0] >= 10 and budget[1] * 1000 <= budget[0]
        # what was planted, as the oracle's rows hold it: anchors 0 and L - 2 of the last probe, the ambiguous allele, and the private one called in sample 0 only
        at = int(np.sum(lens[:4]))
        assert all(any(k[0] == at for k in rows[r].count) and any(k[0] == at + lens[4] - 2 for k in rows[r].count) for r in range(4))
        assert any(q["ambiguous"] for q in rows[2].records)
        private = [c for c in IC.call_session(rows, True, P1)[0][1] if c["length"] == 2 and c["bases"] == I.pack(b"GC") and c["alt"] == 4]
        assert len(private) == 1 and private[0]["bg_alt"] == 0
    finally:
        a.close()


def test_rows_of_0_and_65_records_the_other_calls_and_the_timing(genome):
    """Sample 0 shows no insertion, sample 1 exactly 65 alleles, sample 2 some of them again.  A gapped pileup, a variant call and a locus pileup made before the
    pool and the insertion calls return the same bytes after them; index 16 is set by the pool and by a call, indices 4-15 by neither."""
    rng = np.random.default_rng(823)
    mols, arms = cut_probes(genome, [129, 90])
    barcodes = draw_barcodes(rng, 3, 8)
    strings = [b"G", b"C", b"GG", b"GC", b"CG", b"CC", b"GGG", b"GGC", b"GCG", b"GCC", b"CGG", b"CGC", b"CCG", b"CCC"]
    sites = [(p, t) for p, M in enumerate(mols) for t in quiet_sites(M, ARM + 1, len(M) - ARM)[:4]]
    alleles = [(p, t, X) for p, t in sites for X in strings][:65]
    assert len(alleles) == 65
    L = Lane(rng)
    for s in range(3):
        for M in mols:
            for k in range(6):
                L.molecule(M, len(M), len(M), index=barcodes[s], qual=ord("I"))
    for k, (p, t, X) in enumerate(alleles):
        Mv = with_insert(mols[p], t, X)
        variant(L, mols[p], Mv, Mv, len(Mv), len(Mv), qual=ord("I"), index=barcodes[1])
        if k % 5 == 0:
            variant(L, mols[p], Mv, Mv, len(Mv), len(Mv), qual=ord("I"), index=barcodes[2])
    lens = [len(m) for m in mols]
    a = _accel()
    try:
        got, want = session(a, arms, L.shuffled(), barcodes)
        assert got == want
        rows = IC.session_rows(got, mols, 4, 1, 0, 4)
        assert [len(r.records) for r in rows] == [0, 65, 13, 0]
        params = capi.CallParams(min_depth=1, min_alt=1, min_q=0)
        plan = np.arange(sum(lens), dtype=np.int64) * 4

        def others():
            a.consensus_call_pool(mols, lens, 1, 0, 4)
            a.consensus_locus_plan(plan, b"".join(mols))
            out = [a.consensus_pileup_gapped(mols, lens, r, 1, 0, 4) for r in range(3)] + [a.consensus_call(1, params), a.consensus_locus_pileup(mols, lens, 1, 1, 0, 4)]
            return [[x.tobytes() if isinstance(x, np.ndarray) else x for x in o] for o in out]

        before = others()
        n_variant_calls = len(a.consensus_call(1, params)[1])
        p = dict(P1, min_depth=1, min_alt=1)
        a.set_timing(True)
        assert a.last_kernel_ms(16) < 0
        seen = [a.last_kernel_ms(k) for k in range(4, 16)]
        totals = a.consensus_insertion_pool(mols, lens, 1, 0, 4, p["bg_max_ppm"])
        assert a.last_kernel_ms(16) > 0 and [a.last_kernel_ms(k) for k in range(4, 16)] == seen
        compare_pool(a, rows, 3, totals, p["bg_max_ppm"])
        assert totals["entries"] == 78 and totals["alleles"] == 65
        budget = [0, 0]
        oracle = IC.call_session(rows, True, p)
        for r in (1, 0, 3, 2):
            compare_call(a, r, oracle[r], p, budget)
            assert a.last_kernel_ms(16) > 0 and [a.last_kernel_ms(k) for k in range(4, 16)] == seen
        assert budget[0] >= 65 and budget[1] * 1000 <= budget[0]
        a.set_timing(False)
        assert len(a.call_fetch(n_variant_calls)) == n_variant_calls                                          # the variant calls of the handle are still the last variant call's
        assert others() == before
        a.consensus_insertions(mols, lens, 1, 1, 0, 4)                                                          # a plain insertions call leaves the pool where it is
        compare_pool(a, rows, 3, totals, p["bg_max_ppm"])
    finally:
        a.close()


def test_without_barcodes_zero_groups_and_the_state_errors(genome):
    rng = np.random.default_rng(829)
    mols, arms = cut_probes(genome, [90, 64])
    L = Lane(rng)
    for M in mols:
        for k in range(12):
            Mv = with_insert(M, quiet_sites(M, ARM + 1, len(M) - ARM)[0], b"GC") if k % 4 == 0 else M
            variant(L, M, Mv, Mv, len(Mv), len(Mv), qual=ord("I"))
    ext, lig, eq, lq, idx = L.shuffled()
    n, lens = len(arms), np.array([len(m) for m in mols], dtype=np.int32)
    seq = b"".join(mols)
    a = _accel()
    try:
        lib, h = a.lib, a.h
        i32p = capi.C.POINTER(capi.C.c_int32)
        prm = capi.CallParams(min_depth=1, min_alt=1, min_q=0)
        ptot, ctot = capi.InsertionPoolTotals(), capi.CallTotals()
        pool = lambda seq_=seq, n_=n, W=4, bg=200000: lib.mipgen_accel_reads_consensus_insertion_pool(h, seq_, lens.ctypes.data_as(i32p), n_, 1, 0, W, bg, capi.C.byref(ptot))
        call = lambda row=0, prm_=prm: lib.mipgen_accel_reads_consensus_insertion_call(h, row, capi.C.byref(prm_) if prm_ is not None else None, None, None, None,
                                                                                      capi.C.byref(ctot))
        pfetch = lambda k: lib.mipgen_accel_insertion_pool_fetch(h, np.zeros(max(k, 1), dtype=capi.INSERTION_POOL_RECORD_DTYPE).ctypes.data, k, None)
        assert pool() == E_STATE and b"holds no consensus reads" in lib.mipgen_accel_last_error() and call() == E_STATE and pfetch(0) == E_STATE
        arr = capi.probe_array(arms)
        assert lib.mipgen_accel_reads_open_consensus(h, arr, n, 8, 0, 0, None, 0, 0, 0) == 0
        assert lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, None) == 0
        assert call() == E_STATE and b"no insertion pool" in lib.mipgen_accel_last_error() and pfetch(0) == E_STATE
        # a session without groups: an empty pool, and a call that tests nothing
        assert pool() == 0 and (ptot.rows, ptot.entries, ptot.alleles) == (1, 0, 0) and pfetch(0) == 0 and pfetch(1) == E_INVALID
        assert call() == 0 and (ctot.tested, ctot.candidates, ctot.calls) == (0, 0, 0) and lib.mipgen_accel_insertion_call_fetch(h, None, 0) == 0
        got = a.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=TAGS)[4]
        assert call() == E_STATE and pfetch(0) == E_STATE                                                       # new reads: the pool went with the old ones
        for kw in ({"seq_": None}, {"n_": n + 1}, {"W": 0}, {"W": 16}, {"bg": -1}, {"bg": 1000001}):
            assert pool(**kw) == E_INVALID, kw
        assert call() == E_STATE                                                                                # a refused pool leaves none
        # the one row of a session without barcodes is inside its own pool
        rows = IC.session_rows(got, mols, 1, 1, 0, 4)
        p = dict(P1, min_depth=1, min_alt=1)
        totals = a.consensus_insertion_pool(mols, [int(v) for v in lens], 1, 0, 4, p["bg_max_ppm"])
        compare_pool(a, rows, 1, totals, p["bg_max_ppm"])
        budget = [0, 0]
        counts, anchors, it, recs, ct = compare_call(a, 0, IC.call_session(rows, False, p)[0], p, budget)
        assert len(recs) == 2 and recs["bg_alt"].tolist() == [0, 0] and recs["bg_depth"].tolist() == [0, 0] and budget[1] == 0    # 3 of 12 is above 20 %: never in; nothing else is
        assert call(row=1) == E_INVALID and call(row=-1) == E_INVALID and call(prm_=None) == E_INVALID and call(prm_=capi.CallParams(min_depth=0)) == E_INVALID
        assert call(prm_=capi.CallParams(bg_max_ppm=1)) == E_STATE and b"insertion pool was built with" in lib.mipgen_accel_last_error()
        assert len(a.insertion_call_fetch(2)) == 2                                                              # a refused call leaves the records of the last one
        assert lib.mipgen_accel_reads_open(h, arr, n, 8, 0, 0) == 0 and call() == E_STATE and pfetch(0) == E_STATE
        assert lib.mipgen_accel_reads_finish(h, None, None, None) == 0
    finally:
        a.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_barcodes", [False, True])
def test_cli_equals_the_oracle(tmp_path, with_barcodes):
    """A small table on both strands and FASTQ with planted insertions: the -call_insertions file byte for byte and the new last stderr line; the -pileup file, the
    -pileup_insertions file, the -call file and every other stderr line are those of the run without the option."""
    g = H.golden_genome()
    rng = np.random.default_rng(839 + with_barcodes)
    t_rows, at = [], 5000
    for k in range(4):
        first = clean_window(g, at, 140)
        t_rows.append(synthetic_row(g, first, first + (130, 121, 140, 64)[k] - 1, b"+" if k % 2 else b"-", arm=20 + k % 3))
        at = first + 400
    with open(tmp_path / "table.txt", "wb") as fh:
        fh.write(HEADER.encode() + b"".join(b"\t".join(r) + b"\n" for r in t_rows))
    mols = [r[6] + r[13] + r[10] for r in t_rows]
    arms = [(r[6], r[10]) for r in t_rows]
    barcodes = draw_barcodes(rng, 3, 8)
    labels = ["sample_a", "sample_b", "sample_c"]
    ext, lig, eq, lq, idx = [], [], [], [], []
    for p, M in enumerate(mols):
        for k in range(24):
            tag = random_tag(rng, 8)
            s = k % 3
            Mv = with_insert(M, 30 + p, (b"GAT", b"T")[p % 2]) if k in (0, 3, 6, 9, 1) else with_insert(M, 40 + p, b"C") if k % 8 == 7 else M
            index = barcodes[s] if k < 22 else random_tag(rng, 8)
            e, l = tag[:5] + (Mv + PAD)[:95], tag[5:] + (R.revcomp(Mv) + PAD)[:97]
            ext.append(e); lig.append(l); idx.append(index)
            eq.append(b"I" * len(e)); lq.append(b"I" * len(l))
    write_fastq_q(tmp_path / "ext.fq", ext, eq); write_fastq_q(tmp_path / "lig.fq", lig, lq)
    write_fastq_q(tmp_path / "i1.fq", idx, [b"I" * 8] * len(idx))
    with open(tmp_path / "samples.tsv", "wb") as fh:
        fh.write(b"\n".join(l.encode() + b"\t" + b for l, b in zip(labels, barcodes)) + b"\n")
    common = [COUNT_BIN, "-tag_sizes", "5,3", "-reads", "ext.fq", "lig.fq", "table.txt", "-o", "counts.tsv"] + (
        ["-barcodes", "samples.tsv", "-index_reads", "i1.fq"] if with_barcodes else [])
    want = CONS.consensus_reads(arms, ext, lig, eq, lq, idx if with_barcodes else None, barcodes if with_barcodes else None, 0, (5, 3))
    assert want[2]["assigned"] == len(ext)
    lab = labels if with_barcodes else None
    p = CR.params(min_depth=4, min_alt=2, min_q=10, a0=1, n0=1000, bg_max_ppm=300000)
    opts = ["-call_min_depth", "4", "-call_min_alt", "2", "-call_min_q", "10", "-call_background_max_ppm", "300000"]
    ins = ["-pileup_indels", "4", "-pileup_insertions"]
    text, line, excluded = IC.calls_file(want[4], t_rows, lab, p, 1, 0, 4)
    assert excluded == 0 and text.count(b"\n") > 2 and b"\t-\t" in text and b"\t+\t" in text
    base = _run(common + ["-pileup", "pile0.tsv"] + ins + ["ins0.tsv"], str(tmp_path))
    assert base.returncode == 0, base.stderr.decode()
    run = _run(common + ["-pileup", "pile.tsv"] + ins + ["ins.tsv", "-call_insertions", "icalls.tsv"] + opts, str(tmp_path))
    assert run.returncode == 0, run.stderr.decode()
    assert open(tmp_path / "icalls.tsv", "rb").read() == text
    assert run.stderr.decode() == base.stderr.decode() + line
    assert open(tmp_path / "pile.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read() == G.pileup_file(want[4], t_rows, lab, 1, 0, 4)[0]
    assert open(tmp_path / "ins.tsv", "rb").read() == open(tmp_path / "ins0.tsv", "rb").read() == I.insertions_file(want[4], t_rows, lab, 1, 0, 4)[0]
    # with -call beside it: the call route runs unchanged, and the insertion call of a row feeds INS and ICALLS
    base = _run(common + ["-pileup", "pile0.tsv", "-call", "calls0.tsv"] + ins + ["ins0.tsv"] + opts, str(tmp_path))
    assert base.returncode == 0, base.stderr.decode()
    run = _run(common + ["-pileup", "pile.tsv", "-call", "calls.tsv"] + ins + ["ins2.tsv", "-call_insertions", "icalls2.tsv"] + opts, str(tmp_path))
    assert run.returncode == 0, run.stderr.decode()
    assert open(tmp_path / "icalls2.tsv", "rb").read() == text and run.stderr.decode() == base.stderr.decode() + line
    assert open(tmp_path / "ins2.tsv", "rb").read() == open(tmp_path / "ins0.tsv", "rb").read()
    assert open(tmp_path / "pile.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read()
    assert open(tmp_path / "calls.tsv", "rb").read() == open(tmp_path / "calls0.tsv", "rb").read()
