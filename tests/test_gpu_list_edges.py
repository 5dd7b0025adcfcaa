"""GPU: the two list kernels (k_candidates, a workgroup per entry; k_features_batch, a wavefront per entry) over both sources of a list entry
(probes given by sequence, candidates addressed by coordinates) at the shapes where their shared front can go wrong: arms of 1, 2, 63 and 64
bases (one wavefront stages them, lane i on base i), inserts with no 2- / 3-mer, inserts on each side of one and two MAX_INSERT = 1,024-base
pieces and of the two bases of look-ahead, a non-ACGT byte under a window that crosses the piece boundary, both strands, the first and the last
constructible scan position of a region, masked and SNP-class bases across an arm.  Everything is equality of bit patterns, except the logistic
score against the reference (2 ulp and 1e-5: the figures of tests/test_gpu_probes.py::test_scores_against_the_reference)."""
import os

import numpy as np
import pytest

from mipgen_amd import capi, synth
from oracle import pyoracle as po
from tests import helpers as H
from tests.test_gpu_probes import MIDDLE, MODEL, N_LRC_ROWS, as_probe_tuples, is_guarded, need_ref, ref_features

pytestmark = pytest.mark.gpu
ARMS = (1, 2, 63, 64)
INSERTS = (1, 2, 3, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050)
BOUNDARY = (1022, 1023, 1024, 1025)             # oriented insert offsets around the end of the first staged piece
CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def edge_probes():
    """Every pair of arm lengths with every insert length, strands alternating; then every insert that reaches past the first piece with a non-ACGT
    byte at each oriented offset of BOUNDARY; a few guards.  Forward strings, as tests.test_gpu_probes.random_probes returns them."""
    rng = np.random.default_rng(31)
    g = synth.random_genome(6000, 41)
    out = []

    def cut(e, l, ss, strand, t):
        p = 200 + 7 * (t % 50)
        ext = g[p - e:p] if strand == 0 else g[p + ss:p + ss + e]
        lig = g[p + ss:p + ss + l] if strand == 0 else g[p - l:p]
        return {"strand": strand, "ext": ext, "lig": lig, "ins": g[p:p + ss], "middle": MIDDLE, "ec": int(rng.choice([1, 2, 19, 100, 101, 70000])),
                "lc": int(rng.choice([1, 3, 100, 1000])), "lrc": int(rng.integers(-1, N_LRC_ROWS))}

    for e in ARMS:
        for l in ARMS:
            for ss in INSERTS:
                out.append(cut(e, l, ss, len(out) & 1, len(out)))
    n_plain = len(out)
    for ss in INSERTS:
        for off in BOUNDARY:
            if off >= ss:
                continue
            pr = cut(ARMS[len(out) % 4], ARMS[(len(out) // 4) % 4], ss, len(out) & 1, len(out))
            ins = bytearray(pr["ins"])
            ins[off if pr["strand"] == 0 else ss - 1 - off] = b"NnR-"[len(out) % 4]          # (an N or a '-' in the insert is no guard)
            pr["ins"] = bytes(ins)
            out.append(pr)
    n_planted = len(out) - n_plain
    for k, (field, byte) in enumerate((("ext", b"N"), ("lig", b"N"), ("ext", b"-"), ("lig", b"-"), ("middle", None), ("ext", b"N"))):
        pr = cut(ARMS[k % 4], ARMS[3 - k % 4], INSERTS[3 + k], k & 1, len(out))
        if field == "middle":
            pr["middle"] = MIDDLE[:9] + b"-" + MIDDLE[10:]
        else:
            s = bytearray(pr[field]); s[len(s) // 2] = byte[0]; pr[field] = bytes(s)
        out.append(pr)
    assert n_plain == 176 and n_planted == 1 + 2 + 3 + 4 + 4 * 4
    return out


def counts_of(tup):
    """The integer features of a probe as plain Python counts of its oriented strings (mipgen_candidate_ints: mipgen_accel.h)."""
    ext, lig, ins = tup[0], tup[1], tup[2]
    d = {}
    for name, s in (("ext", ext), ("lig", lig), ("ins", ins)):
        for b in b"ACGT":
            d[f"{name}_{chr(b).lower()}"] = s.count(bytes([b]))
    d["junction"] = 4 * CODE[lig[0]] + CODE[lig[1]] if len(lig) >= 2 and lig[0] in CODE and lig[1] in CODE else 255
    d["scan_size"] = len(ins)
    return d


@need_ref
def test_probes_at_the_edges_against_the_reference():
    """All 192 doubles of every edge probe equal SVMipv4::get_parameters' as a bit pattern through k_candidates (features asked with a logistic score
    and the integer features) and through k_features_batch (an SVR list of >= 256 entries: the probes twice, the repeats identical); logistic scores
    within 2 ulp and 1e-5 of the reference's; the integer features equal plain counts of the oriented strings."""
    R = po.refdrv()
    probes = edge_probes()
    lrc_rows = np.random.default_rng(8).uniform(0, 0.3, (N_LRC_ROWS, 44))
    want = ref_features(R, probes, lrc_rows)
    want_log = np.array([R.ref_logistic(pr["strand"], pr["ext"], pr["lig"], pr["ins"], pr["ec"], pr["lc"], pr["middle"]) for pr in probes])
    tup = as_probe_tuples(R, probes)
    guards = np.array([is_guarded(pr) for pr in probes])
    assert guards.sum() == 6
    n = len(tup)
    assert 2 * n >= 256
    acc = capi.Accel(capi.make_params(152, 162, score_method=capi.SCORE_SVR))
    try:
        acc.load_model_file(MODEL)
        s_log, f_cand, ints = acc.score_probes(tup, capi.SCORE_LOGISTIC, lrc=lrc_rows, want_features=True, want_ints=True)       # k_candidates
        _, f_batch, _ = acc.score_probes(tup + tup, capi.SCORE_SVR, lrc=lrc_rows, want_features=True)                            # k_features_batch
    finally:
        acc.close()
    assert np.array_equal(bits(f_batch[:n]), bits(f_batch[n:]))
    for name, got in (("k_features_batch", f_batch[:n]), ("k_candidates", f_cand)):
        bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (name, [(int(b), len(tup[b][0]), len(tup[b][1]), len(tup[b][2]), np.nonzero(bits(got[b]) != bits(want[b]))[0][:6]) for b in bad[:5]])
    d_log = np.abs(s_log - want_log)
    ulp = d_log / np.spacing(np.maximum(np.abs(want_log), 1e-300))
    print(f"\nedge probes vs reference: logistic max |d| {d_log.max():.3e}, max {ulp.max():.1f} ulp")
    assert np.all(d_log <= 1e-5) and ulp.max() <= 2.0
    assert np.all(s_log[guards] == -1000.0) and np.all(s_log[~guards] != -1000.0)
    for i, t in enumerate(tup):
        for f, v in counts_of(t).items():
            assert getattr(ints[i], f) == v, (i, f, getattr(ints[i], f), v)
        assert ints[i].flags == capi.FLAG_VALID | (capi.FLAG_GUARD if guards[i] else 0)
        assert (ints[i].ext_copy, ints[i].lig_copy, ints[i].masked_n, ints[i].snp_count) == (probes[i]["ec"], probes[i]["lc"], 0, 0)


def test_coordinates_at_the_edges_agree_across_kernels_and_sources():
    """One 3 kb region that starts at base 1: arm pairs (2,2), (2,64), (64,2), (64,64), the insert lengths of INSERTS as far as the region holds them,
    both strands, at the first and the last constructible scan position and at two positions whose arms cross masked and SNP-class bases.  Features
    and records of k_candidates equal those of k_features_batch; both equal the probe route fed the host-sliced oriented strings, in the fields
    tests/test_gpu_probes.py::test_agreement_with_the_coordinate_route compares (features, integer features, logistic and SVR scores)."""
    L = 3000
    genome = synth.random_genome(L, 43)
    pairs = [(2, 2), (2, 64), (64, 2), (64, 64)]
    # (a list candidate carries its own capture size: the list scorers take any, on the design's grid of sizes or not - the grid only sizes the dense arrays)
    P = capi.make_params(129, 2050 + 128, score_method=capi.SCORE_SVR, capture_increment=53, arm_pairs=pairs)
    masked = bytearray(genome)
    snp = np.zeros(L, dtype=np.uint8)
    for a, b in ((60, 70), (1480, 1500), (2990, 2996)):                    # 1-based positions [a, b)
        masked[a - 1:b - 1] = b"N" * (b - a)
    snp[[39, 1389, 2979]] = 1
    snp[[49, 1394, 1395, 2969]] = 2
    lrc_row = np.linspace(0.01, 0.3, 44)
    rd = capi.RegionData(1400, 1600, 1, genome, masked=bytes(masked), snp_class=snp, lrc=lrc_row, chrom="1", label="edges", start=1400, stop=1600)
    cands = []
    for e, l in pairs:
        for ss in INSERTS:
            C = ss + e + l
            first, last = max(e, l) + 1, L - C + min(e, l) + 1             # constructed(): mip_record.h (mipgen.cpp:443-444)
            if last < first:
                continue
            for p in sorted({first, last} | {q for q in (66, 1500) if first <= q <= last}):
                for strand in (0, 1):
                    cands.append((0, p, C, e, l, strand))
    assert len(cands) >= 256 and {c[2] - c[3] - c[4] for c in cands} >= set(INSERTS[:7])
    tup = []
    for (_, p, C, e, l, strand) in cands:
        ss = C - e - l
        ext_start, lig_start = (p - e, p + ss) if strand == 0 else (p + ss, p - l)
        ext, lig, ins = po.orient(strand, genome[ext_start - 1:ext_start - 1 + e], genome[lig_start - 1:lig_start - 1 + l], genome[p - 1:p - 1 + ss])
        assert (len(ext), len(lig), len(ins)) == (e, l, ss)
        tup.append((ext, lig, ins, lig + MIDDLE + ext, 1, 1, 0))             # no copy table: every oligo has one copy
    acc = capi.Accel(P)
    try:
        acc.load_model_file(os.path.join(H.GOLDEN, "models", "svr_syn_200.model"))
        acc.upload([rd])
        c_log, c_rec, c_feat, c_ints = acc.score_candidates(cands, capi.SCORE_LOGISTIC, want_features=True, want_ints=True)      # k_candidates
        c_svr, c_rec_b, c_feat_b, _ = acc.score_candidates(cands, capi.SCORE_SVR, want_features=True)                            # k_features_batch + k_svr_gemm
        c_svr_short = acc.score_candidates(cands[:200], capi.SCORE_SVR)[0]
        p_log, p_feat, p_ints = acc.score_probes(tup, capi.SCORE_LOGISTIC, lrc=lrc_row[None, :], want_features=True, want_ints=True)
        p_svr, p_feat_b, _ = acc.score_probes(tup, capi.SCORE_SVR, lrc=lrc_row[None, :], want_features=True)
        p_svr_short = acc.score_probes(tup[:200], capi.SCORE_SVR, lrc=lrc_row[None, :])[0]
    finally:
        acc.close()
    assert all(c_ints[i].flags & capi.FLAG_VALID for i in range(len(cands)))
    assert sum(c_ints[i].masked_n > 0 for i in range(len(cands))) >= 8 and sum(c_ints[i].snp_count > 0 for i in range(len(cands))) >= 8
    assert any(c_ints[i].flags & capi.FLAG_MASKING for i in range(len(cands))) and any(c_ints[i].flags & capi.FLAG_SNP for i in range(len(cands)))
    assert np.array_equal(bits(c_feat), bits(c_feat_b)) and np.array_equal(c_rec, c_rec_b)
    assert np.array_equal(bits(p_feat), bits(c_feat)) and np.array_equal(bits(p_feat_b), bits(c_feat_b))
    for i, t in enumerate(tup):
        for f in capi.INTS_FIELDS:
            if f in ("masked_n", "snp_count"):                              # from tables a probe does not carry
                continue
            got, want = getattr(p_ints[i], f), getattr(c_ints[i], f)
            if f == "flags":
                want &= capi.FLAG_VALID | capi.FLAG_GUARD
            assert got == want, (i, f, cands[i])
        for f, v in counts_of(t).items():
            assert getattr(c_ints[i], f) == v, (i, f, cands[i])
    assert np.array_equal(bits(p_log), bits(c_log))
    assert np.array_equal(bits(p_svr), bits(c_svr))
    assert np.array_equal(bits(p_svr_short), bits(c_svr_short))
