"""GPU: pileup and calls per genome locus end to end from reads (mipgen_accel_reads_consensus_locus_plan / _locus_pileup / _locus_call_pool / _locus_call,
`mipgen_count -pileup_loci / -call_loci`).  Six probes tile 400 bases of a golden genome with half overlap on alternating strands; three samples
and undetermined.  Planted: a substitution of sample_a split over two probes so that neither probe calls it and the locus does, a two-base deletion of sample_b in
an overlap, and a substitution of sample_c on a base that is the arm of one probe and the target of the one before.  Every comparison is exact equality against
tests/locus_ref.py on the tables tests/pileup_ref.py / tests/gapped_ref.py make of the groups, after the one exclusion of the call model (a candidate whose exact
score lies within 1e-6 of an integer is dropped from both sides, at most 1 in 1,000)."""
import faulthandler
import json

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CALL
from tests import consensus_ref as CR
from tests import gapped_ref as G
from tests import helpers as H
from tests import locus_ref as LR
from tests import pileup_ref as PR
from tests import reads_ref as R
from tests.test_gpu_pileup import COUNT_BIN, TAGS, Lane, _run, write_fastq_q
from tests.test_gpu_reads import TABLES, _accel, random_tag
from tests.test_gpu_samples import GOLDEN_PLAIN, clean_reads_uneven_depth_inputs, draw_barcodes, plain_session_digest
from tests.test_pileup_cpu import clean_window, synthetic_row
from tests.test_reads_cpu import HEADER

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE = -1, -6
LENGTH, STEP, ARM_LEN, DEPTH, W = 114, 57, 16, 30, 8
LABELS = ["sample_a", "sample_b", "sample_c"]
COMP = {65: 84, 67: 71, 71: 67, 84: 65}


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


def where(row, position):
    """The template position at which the molecule of table row `row` shows genome position `position`."""
    return int(row[4]) - position if row[17] == b"-" else position - int(row[3])


def shown(row, base):
    """What the molecule of `row` shows where the plus strand has `base`."""
    return COMP[base] if row[17] == b"-" else base


def build_design():
    """The six table rows - probe k spans first + 57 k .. first + 57 k + 113, its target the offsets 16 .. 97 of that - and the three planted sites in genome terms:
    (substitution position, alt), the first deleted position, (arm-and-target position, alt)."""
    g = H.golden_genome()
    first = clean_window(g, 5000, 5 * STEP + LENGTH)
    rows = [synthetic_row(g, first + k * STEP, first + k * STEP + LENGTH - 1, b"-" if k % 2 else b"+", arm=ARM_LEN) for k in range(6)]
    other = lambda position, d: b"ACGT"[(b"ACGT".index(g[position - 1]) + d) & 3]
    sub = first + 140                                                        # in the targets of probes 1 and 2 (first + 130 .. first + 154 is in both)
    dele = first + 248                                                       # in the targets of probes 3 and 4 (first + 244 .. first + 268)
    i = dele - 1
    while g[i] == g[i + 2] or g[i + 1] == g[i + 3] or g[i - 1] == g[i + 1] or g[i] == g[i - 2]:      # (a deletion that can slide along a repeat has no single placement)
        dele, i = dele + 1, i + 1
    assert dele + 1 <= first + 262
    arm = first + 290                                                        # in the ligation arm of probe 5 (first + 285 .. first + 300) and in the target of probe 4 alone
    return g, rows, (sub, other(sub, 1)), dele, (arm, other(arm, 2))


def build_lane(rng, rows, sites, barcodes):
    """DEPTH molecules per (sample, probe), a third of that undetermined; the planted evidence of build_design."""
    (sub, sub_alt), dele, (arm, arm_alt) = sites
    mols = [r[6] + r[13] + r[10] for r in rows]
    L = Lane(rng)
    for s in range(4):
        for p, (row, M) in enumerate(zip(rows, mols)):
            for k in range(DEPTH // 3 if s == 3 else DEPTH):
                index = barcodes[s] if s < 3 else random_tag(rng, 8)
                subs, edit = [], None
                if s == 0 and p in (1, 2) and k < 2:                         # 2 + 2 alt molecules of 30 + 30
                    subs = [(where(row, sub), shown(row, sub_alt))]
                if s == 2 and p == 4 and k < 12:                             # the sample's DNA at a base that is probe 5's arm: probe 5's own reads show the oligo there
                    subs = [(where(row, arm), shown(row, arm_alt))]
                if s == 1 and p in (3, 4) and k < 6:                         # two bases deleted
                    t = min(where(row, dele), where(row, dele + 1))
                    deleted = M[:t] + M[t + 2:]
                    edit = lambda m, e, l, eq, lq, d=deleted: (e[:TAGS[0]] + d, R.revcomp(d), b"I" * (TAGS[0] + len(d)), b"I" * len(d))
                L.molecule(M, len(M), len(M), subs=subs, qual=ord("I"), index=index, member_edit=edit)
    return mols, L


@pytest.fixture(scope="module")
def lane():
    """The design, the reads and everything the oracles make of them, computed once: the count tables of the four rows without and with indels, the plans of both
    -loci_parts, the merged tables."""
    g, rows, sites = (lambda d: (d[0], d[1], d[2:]))(build_design())
    rng = np.random.default_rng(4151)
    barcodes = draw_barcodes(rng, 3, 8)
    mols, L = build_lane(rng, rows, sites, barcodes)
    cols = L.shuffled()
    arms = [(r[6], r[10]) for r in rows]
    ext, lig, eq, lq, idx = cols
    groups = CR.consensus_reads(arms, ext, lig, eq, lq, idx, barcodes, 0, TAGS)[4]
    lens, n = [len(m) for m in mols], len(mols)
    tables = {0: [PR.pileup(groups, lens, n, r, 1, 0)[0] for r in range(4)], W: [G.pileup(groups, mols, n, r, 1, 0, W)[0] for r in range(4)]}
    plans = {parts: LR.build_plan(rows, parts) for parts in ("target", "all")}
    return dict(g=g, rows=rows, sites=sites, barcodes=barcodes, mols=mols, lens=lens, arms=arms, cols=cols, groups=groups, tables=tables, plans=plans)


def open_session(acc, lane):
    ext, lig, eq, lq, idx = lane["cols"]
    assert acc.consensus_reads(lane["arms"], ext, lig, eq, lq, idx, lane["barcodes"], 0, TAGS, chunks=2)[4] == lane["groups"]


def locus_index(lane, parts, position):
    return lane["plans"][parts][1].index((b"1", position))


# ---- the pileup per locus ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", ["target", "all"])
@pytest.mark.parametrize("max_indel", [0, W])
def test_locus_pileup_equals_the_oracle(acc, lane, max_indel, parts):
    open_session(acc, lane)
    mols, lens = lane["mols"], lane["lens"]
    plan, loci, ref, sources = lane["plans"][parts]
    pileup = (lambda r: acc.consensus_pileup_gapped(mols, lens, r, 1, 0, W)) if max_indel else (lambda r: acc.consensus_pileup(lens, r))
    before = [pileup(r) for r in range(4)]
    acc.consensus_locus_plan(plan, ref)
    included = np.array([e >= 0 for e in plan])
    for row in (2, 0, 1, 0, 3):                                                # any order, a row twice, undetermined too
        want = LR.merge(lane["tables"][max_indel][row], plan, len(loci))
        probe, merged, pt, lt = acc.consensus_locus_pileup(mols if max_indel else None, lens, row, 1, 0, max_indel)
        again = acc.consensus_locus_pileup(mols, lens, row, 1, 0, max_indel)
        assert probe.tobytes() == again[0].tobytes() and merged.tobytes() == again[1].tobytes() and (pt, lt) == again[2:]
        assert np.array_equal(probe, lane["tables"][max_indel][row]) and np.array_equal(probe, before[row][0])
        assert {k: pt[k] for k in before[row][1]} == before[row][1]
        assert np.array_equal(merged, want), (row, np.flatnonzero((merged != want).any(axis=1))[:5])
        assert lt == LR.totals(want)
        assert lt["bases"] == int(probe[included, :4].sum()) and lt["discordant"] == int(probe[included, 4].sum())
        if max_indel:
            assert lt["deletions"] == int(probe[included, 5].sum())
    for r in range(4):                                                        # the pileup entry points give what they gave before
        counts, totals = pileup(r)
        assert np.array_equal(counts, before[r][0]) and totals == before[r][1]


def test_the_planted_evidence_is_where_the_design_says(lane):
    """(Oracle only.)  The split substitution, the deletion and the arm base in the per-probe tables and in the merged ones."""
    (sub, sub_alt), dele, (arm, arm_alt) = lane["sites"]
    rows, lens = lane["rows"], lane["lens"]
    at = np.cumsum([0] + lens)
    col = lambda row, base: b"ACGT".index(shown(row, base))
    t0 = lane["tables"][0]
    for p in (1, 2):
        assert t0[0][at[p] + where(rows[p], sub)][col(rows[p], sub_alt)] == 2 and t0[0][at[p] + where(rows[p], sub)][:4].sum() == DEPTH
    plan, loci, ref, sources = lane["plans"]["target"]
    l = locus_index(lane, "target", sub)
    assert sources[l] == 2 and LR.merge(t0[0], plan, len(loci))[l][b"ACGT".index(sub_alt)] == 4
    # the arm base: probe 4 shows the sample's alt, probe 5 its own oligo; only probe 4's target counts under `target`, both lines under `all`
    l = locus_index(lane, "target", arm)
    x4, x5 = at[4] + where(rows[4], arm), at[5] + where(rows[5], arm)
    assert where(rows[5], arm) >= LENGTH - ARM_LEN and ARM_LEN <= where(rows[4], arm) < LENGTH - ARM_LEN
    assert t0[2][x4][col(rows[4], arm_alt)] == 12 and t0[2][x5][col(rows[5], arm_alt)] == 0 and t0[2][x5][:4].sum() == DEPTH
    assert sources[l] == 1 and LR.merge(t0[2], plan, len(loci))[l].tolist() == [int(v) for v in (t0[2][x4][[3, 2, 1, 0, 4]] if rows[4][17] == b"-" else t0[2][x4])]
    plan_all, loci_all, _, sources_all = lane["plans"]["all"]
    l_all = locus_index(lane, "all", arm)
    assert sources_all[l_all] == 2 and LR.merge(t0[2], plan_all, len(loci_all))[l_all][:4].sum() == 2 * DEPTH
    # the deletion: 6 molecules of probe 3 and 6 of probe 4 on both deleted bases, 12 at the locus
    tw = lane["tables"][W]
    merged = LR.merge(tw[1], plan, len(loci))
    for position in (dele, dele + 1):
        assert [tw[1][at[p] + where(rows[p], position)][5] for p in (3, 4)] == [6, 6] and merged[locus_index(lane, "target", position)][5] == 12


# ---- calls per locus -----------------------------------------------------------------------------------------------------------------------------------------
def check_locus_row(acc, lane, tables, plan, loci, ref, pool, row, p):
    """consensus_locus_call of one row, twice: its probe counts are the pileup's, its locus counts, records and totals the oracle's."""
    want = LR.merge(tables[row], plan, len(loci))
    totals, cands = CALL.call_cells(want, pool, ref, row < 3, p)
    assert totals["excluded"] * 1000 <= max(totals["candidates"], 1), (row, totals)
    probe, merged, records, got = acc.consensus_locus_call(row, capi.CallParams(**p))
    probe2, merged2, records2, got2 = acc.consensus_locus_call(row, capi.CallParams(**p))
    assert probe.tobytes() == probe2.tobytes() and merged.tobytes() == merged2.tobytes() and records.tobytes() == records2.tobytes() and got == got2
    assert np.array_equal(probe, tables[row]) and np.array_equal(merged, want)
    assert {k: got[k] for k in ("tested", "too_deep", "candidates")} == {k: totals[k] for k in ("tested", "too_deep", "candidates")}, row
    assert CALL.drop_excluded(records, cands) == CALL.kept_calls(cands, p), row
    assert totals["excluded"] or got["calls"] == len(records) == totals["calls"]
    return [(int(r["pos"]), int(r["allele"])) for r in records]


@pytest.mark.parametrize("max_indel", [0, W])
def test_locus_calls_equal_the_oracle_and_find_what_no_probe_finds(acc, lane, max_indel):
    open_session(acc, lane)
    mols, lens, tables = lane["mols"], lane["lens"], lane["tables"][max_indel]
    (sub, sub_alt), dele, (arm, arm_alt) = lane["sites"]
    plan, loci, ref, sources = lane["plans"]["target"]
    p = CALL.params()                                                         # the defaults of `mipgen_count -call`
    # per probe, with the existing calls: the split substitution is not called
    acc.consensus_call_pool(mols, lens, 1, 0, max_indel, p["bg_max_ppm"])
    probe_calls = [acc.consensus_call(r, capi.CallParams(**p)) for r in range(4)]
    at = np.cumsum([0] + lens)
    split = {int(at[q]) + where(lane["rows"][q], sub) for q in (1, 2)}
    assert not split & set(probe_calls[0][1]["pos"].tolist())
    # per locus
    acc.consensus_locus_plan(plan, ref)
    acc.consensus_locus_call_pool(mols, lens, 1, 0, max_indel, p["bg_max_ppm"])
    pool = CALL.pool([LR.merge(t, plan, len(loci)) for t in tables[:3]], p["bg_max_ppm"])
    called = {row: check_locus_row(acc, lane, tables, plan, loci, ref, pool, row, p) for row in (2, 0, 1, 0, 3)}
    assert (locus_index(lane, "target", sub), b"ACGT".index(sub_alt)) in called[0]
    assert (locus_index(lane, "target", arm), b"ACGT".index(arm_alt)) in called[2] and called[3] == []
    if max_indel:
        assert {(locus_index(lane, "target", dele), 4), (locus_index(lane, "target", dele + 1), 4)} <= set(called[1])
    pt = acc.consensus_locus_call_pileup_totals()
    assert pt["groups"] == sum(1 for grp in lane["groups"] if grp[0] // 6 == 3)
    # the existing calls give their own results after the locus calls
    for r in range(4):
        counts, records, totals = acc.consensus_call(r, capi.CallParams(**p))
        assert np.array_equal(counts, probe_calls[r][0]) and records.tobytes() == probe_calls[r][1].tobytes() and totals == probe_calls[r][2]


# ---- state ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_refusals(lane):
    mols, lens = lane["mols"], np.array(lane["lens"], dtype=np.int32)
    plan, loci, ref, sources = lane["plans"]["target"]
    plan_all, loci_all, ref_all, _ = lane["plans"]["all"]
    a = _accel()
    try:
        lib, h, C = a.lib, a.h, capi.C
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        arr, seq = np.array(plan, dtype=np.int64), b"".join(mols)
        prm, tot = capi.CallParams(), capi.CallTotals()
        install = lambda plan_=arr, ref_=ref, n_loci=None: lib.mipgen_accel_reads_consensus_locus_plan(
            h, plan_.ctypes.data_as(i64p) if plan_ is not None else None, len(plan_) if plan_ is not None else 1, ref_, len(ref_) if n_loci is None else n_loci)
        pileup = lambda lens_=lens, n=6, W_=0, row=0: lib.mipgen_accel_reads_consensus_locus_pileup(h, seq, lens_.ctypes.data_as(i32p), n, row, 1, 0, W_, None, None, None, None)
        pool = lambda W_=0, bg=200000: lib.mipgen_accel_reads_consensus_locus_call_pool(h, seq, lens.ctypes.data_as(i32p), 6, 1, 0, W_, bg)
        call = lambda row=0: lib.mipgen_accel_reads_consensus_locus_call(h, row, C.byref(prm), None, None, C.byref(tot))
        # nothing is held
        for f in (install, pileup, pool, call):
            assert f() == E_STATE and b"holds no consensus reads" in lib.mipgen_accel_last_error()
        assert lib.mipgen_accel_reads_consensus_locus_call_pileup_totals(h, None) == E_STATE
        ext, lig, eq, lq, idx = lane["cols"]
        a.consensus_reads(lane["arms"], ext, lig, eq, lq, idx, lane["barcodes"], 0, TAGS)
        # reads but no plan
        for f in (pileup, pool, call):
            assert f() == E_STATE and b"no locus plan" in lib.mipgen_accel_last_error()
        # the refusals of a plan leave none
        bad = arr.copy(); bad[40] = len(loci) * 4
        for kw in (dict(plan_=None), dict(ref_=None, n_loci=len(loci)), dict(n_loci=0), dict(n_loci=len(loci) - 1), dict(plan_=bad), dict(plan_=np.array([2], dtype=np.int64)),
                   dict(plan_=np.array([-2], dtype=np.int64))):
            assert install(**kw) == E_INVALID, kw
            assert pileup() == E_STATE
        assert install() == 0
        # a plan, no pool
        assert call() == E_STATE and b"no locus pool" in lib.mipgen_accel_last_error()
        assert pileup() == 0
        # the refusals of the underlying pileup, and a table that is not the plan's
        for kw in (dict(row=4), dict(row=-1), dict(n=5), dict(W_=16), dict(W_=-1), dict(lens_=np.array([114, 114, 114, 114, 114, 0], dtype=np.int32))):
            assert pileup(**kw) == E_INVALID, kw
        assert pileup(lens_=np.array([114, 114, 114, 114, 114, 113], dtype=np.int32)) == E_INVALID and b"the locus plan was installed for 684" in lib.mipgen_accel_last_error()
        assert pool(bg=-1) == E_INVALID and pool(W_=16) == E_INVALID and call() == E_STATE
        assert pool() == 0 and call() == 0
        # another bg_max_ppm than the pool's
        prm.bg_max_ppm = 10 ** 6
        assert call() == E_STATE and b"the locus pool was built with 200000" in lib.mipgen_accel_last_error()
        prm.bg_max_ppm = 200000
        prm.min_alt = 0
        assert call() == E_INVALID
        prm.min_alt = 3
        assert call(4) == E_INVALID and call(3) == 0
        # timing: index 14 and no other
        assert a.last_kernel_ms(14) < 0
        a.set_timing(True)
        assert install() == 0 and a.last_kernel_ms(14) > 0 and call() == E_STATE                   # a plan replaced: the pool is gone
        assert pool() == 0 and a.last_kernel_ms(14) > 0 and call() == 0 and a.last_kernel_ms(14) > 0
        assert pileup(W_=W) == 0 and a.last_kernel_ms(14) > 0 and all(a.last_kernel_ms(k) < 0 for k in (11, 12, 13))
        a.set_timing(False)
        # a plan of another shape replaces the first: the loci are now those of -loci_parts all
        a.consensus_locus_plan(plan_all, ref_all)
        assert call() == E_STATE and pool() == 0 and call() == 0
        merged = a.consensus_locus_pileup(None, lens, 0)[1]
        assert np.array_equal(merged, LR.merge(lane["tables"][0][0], plan_all, len(loci_all)))
        # the next open drops reads, plan and pool
        assert lib.mipgen_accel_reads_open_consensus(h, capi.probe_array(lane["arms"]), 6, 8, 0, 0, None, 0, 0, 0) == 0
        assert call() == E_STATE and pileup() == E_STATE and install() == E_STATE
        assert lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, None) == 0
        assert pileup() == E_STATE and b"no locus plan" in lib.mipgen_accel_last_error()
        assert install() == 0 and pool() == 0 and call() == 0 and (tot.tested, tot.candidates, tot.calls) == (0, 0, 0)      # a session without groups: zero tables
        got = np.full((len(loci), 5), -1, dtype=np.int32)
        lt = capi.LocusTotals()
        assert lib.mipgen_accel_reads_consensus_locus_pileup(h, None, lens.ctypes.data_as(i32p), 6, 0, 1, 0, 0, None, got.ctypes.data_as(i32p), None, C.byref(lt)) == 0
        assert not got.any() and lt.covered == 0
    finally:
        a.close()


def test_the_wrappers_out_of_order_get_the_library_s_refusal(lane):
    """capi's locus wrappers keep the shapes of the plan and the pool they installed; called before either they hand the library NULL tables and raise its STATE error."""
    lens, prm = np.array(lane["lens"], dtype=np.int32), capi.CallParams()
    plan, loci, ref, _ = lane["plans"]["target"]
    a = _accel()
    try:
        for f in (lambda: a.consensus_locus_pileup(None, lens, 0), lambda: a.consensus_locus_call(0, prm)):
            with pytest.raises(capi.AccelError, match=f"error {E_STATE}: .*holds no consensus reads"):
                f()
        ext, lig, eq, lq, idx = lane["cols"]
        a.consensus_reads(lane["arms"], ext, lig, eq, lq, idx, lane["barcodes"], 0, TAGS)
        for f in (lambda: a.consensus_locus_pileup(None, lens, 0), lambda: a.consensus_locus_call(0, prm)):
            with pytest.raises(capi.AccelError, match=f"error {E_STATE}: .*no locus plan"):
                f()
        a.consensus_locus_plan(plan, ref)
        with pytest.raises(capi.AccelError, match=f"error {E_STATE}: .*no locus pool"):
            a.consensus_locus_call(0, prm)
        assert np.array_equal(a.consensus_locus_pileup(None, lens, 0)[1], LR.merge(lane["tables"][0][0], plan, len(loci)))
        a.consensus_locus_call_pool(None, lens)
        assert a.consensus_locus_call(0, prm)[1].shape == (len(loci), 5)
        a.consensus_locus_plan(plan, ref)                                                          # a plan replaced: the wrapper's pool shape goes with the pool
        with pytest.raises(capi.AccelError, match=f"error {E_STATE}: .*no locus pool"):
            a.consensus_locus_call(0, prm)
    finally:
        a.close()


@pytest.mark.parametrize("name,key", TABLES[:1])
def test_a_plain_session_afterwards_is_the_recorded_one(acc, lane, name, key):
    open_session(acc, lane)
    plan, loci, ref, sources = lane["plans"]["target"]
    acc.consensus_locus_plan(plan, ref)
    acc.consensus_locus_call_pool(lane["mols"], lane["lens"])
    acc.consensus_locus_call(0, capi.CallParams())
    t_rows, t_ext, t_lig = clean_reads_uneven_depth_inputs(name, key)
    got = acc.count_reads([(r[6], r[10]) for r in t_rows], t_ext, t_lig, want_assignment=True)
    recorded = json.load(open(GOLDEN_PLAIN))
    assert plain_session_digest(*got) == recorded[f"{name}/{key}"]["sha256"]


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("indels", [0, W])
@pytest.mark.parametrize("with_barcodes", [False, True])
def test_cli_equals_the_oracle(tmp_path, lane, with_barcodes, indels):
    """The design of this file through `mipgen_count`: FILE byte for byte what it is without the new options, LOCI, CALLS and the new stderr lines the oracle's."""
    rows, mols = lane["rows"], lane["mols"]
    ext, lig, eq, lq, idx = lane["cols"]
    with open(tmp_path / "table.txt", "wb") as fh:
        fh.write(HEADER.encode() + b"".join(b"\t".join(r) + b"\n" for r in rows))
    write_fastq_q(tmp_path / "ext.fq", ext, eq); write_fastq_q(tmp_path / "lig.fq", lig, lq)
    write_fastq_q(tmp_path / "i1.fq", idx, [b"I" * 8] * len(idx))
    with open(tmp_path / "samples.tsv", "wb") as fh:
        fh.write(b"\n".join(l.encode() + b"\t" + b for l, b in zip(LABELS, lane["barcodes"])) + b"\n")
    common = [COUNT_BIN, "-tag_sizes", "8,0", "-reads", "ext.fq", "lig.fq", "table.txt", "-o", "counts.tsv"] + (
        ["-barcodes", "samples.tsv", "-index_reads", "i1.fq"] if with_barcodes else [])
    pile_args = ["-pileup_indels", str(indels)] if indels else []
    if with_barcodes:
        tables, lab = lane["tables"][indels], LABELS
    else:                                                                     # one row: every molecule of the lane
        groups = CR.consensus_reads(lane["arms"], ext, lig, eq, lq, None, None, 0, TAGS)[4]
        tables = [G.pileup(groups, mols, 6, 0, 1, 0, indels)[0] if indels else PR.pileup(groups, lane["lens"], 6, 0)[0]]
        lab = None
    p = CALL.params(min_depth=20, min_alt=3, min_q=25)
    call_args = ["-call_min_q", "25"]
    plain = _run(common + ["-pileup", "pile0.tsv"] + pile_args, str(tmp_path))
    assert plain.returncode == 0, plain.stderr.decode()
    # LOCI alone, with the arms: one locus pileup per row
    loci_text, loci_line = LR.loci_file(tables, rows, lab, "all")
    one = _run(common + ["-pileup", "pile1.tsv", "-pileup_loci", "loci1.tsv", "-loci_parts", "all"] + pile_args, str(tmp_path))
    assert one.returncode == 0, one.stderr.decode()
    assert open(tmp_path / "loci1.tsv", "rb").read() == loci_text and loci_text.count(b"\n") > 390
    assert open(tmp_path / "pile1.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read() != b""
    assert one.stderr.decode() == plain.stderr.decode() + loci_line and one.stdout == plain.stdout
    # LOCI and CALLS of the targets: one locus call per row
    loci_text, loci_line = LR.loci_file(tables, rows, lab)
    calls_text, calls_line, excluded = LR.calls_file(tables, rows, lab, p)
    assert excluded == 0 and loci_text.count(b"\n") > 300 and calls_text.count(b"\n") >= 2
    two = _run(common + ["-pileup", "pile2.tsv", "-pileup_loci", "loci2.tsv", "-call_loci", "calls2.tsv"] + pile_args + call_args, str(tmp_path))
    assert two.returncode == 0, two.stderr.decode()
    assert open(tmp_path / "loci2.tsv", "rb").read() == loci_text and open(tmp_path / "calls2.tsv", "rb").read() == calls_text
    assert open(tmp_path / "pile2.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read()
    assert two.stderr.decode() == plain.stderr.decode() + loci_line + calls_line and two.stdout == plain.stdout
    # beside -call: the per-probe files are what they are without the locus options
    text, line, excluded = CALL.calls_file(tables, rows, lab, p)
    assert excluded == 0
    both = _run(common + ["-pileup", "pile3.tsv", "-call", "calls3.tsv", "-pileup_loci", "loci3.tsv", "-call_loci", "lcalls3.tsv"] + pile_args + call_args, str(tmp_path))
    assert both.returncode == 0, both.stderr.decode()
    assert open(tmp_path / "calls3.tsv", "rb").read() == text and open(tmp_path / "pile3.tsv", "rb").read() == open(tmp_path / "pile0.tsv", "rb").read()
    assert open(tmp_path / "loci3.tsv", "rb").read() == loci_text and open(tmp_path / "lcalls3.tsv", "rb").read() == calls_text
    assert both.stderr.decode() == plain.stderr.decode() + line + loci_line + calls_line
    if with_barcodes:                                                         # the split substitution: a line of CALLS, no line of the per-probe file
        sub = b"%d" % lane["sites"][0][0]
        assert any(l.startswith(b"sample_a\t1\t" + sub + b"\t") for l in calls_text.split(b"\n"))
        assert not any(l.startswith(b"sample_a\t") and l.split(b"\t")[3] == sub for l in text.split(b"\n")[1:-1])
