"""GPU: mipgen_accel_train_svr / `mipgen_svr_train`, libsvm's epsilon-SVR trainer on the device, against the reference's own svm_train +
svm_save_model (oracle ref_svm_train_save): the model files must be identical byte for byte.  Training sets are the feature vectors of real
candidates (the reference's SVMipv4::get_parameters) with a smooth target plus noise, as tests/golden/make_golden.py builds its libsvm fixture."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi, synth
from oracle import pyoracle as po
from oracle import run_reference as rr
from tests import helpers as H

pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(not po.have_refdrv(), reason="reference driver (oracle/_ref) not built")
TRAIN_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_svr_train")
MIDDLE = b"CTTCAGCTTCCCGATATCCGACGGTAGTGT"
_dp = C.POINTER(C.c_double)


def training_set(n: int, seed: int, dup_frac: float = 0.0, zero_rows: int = 0):
    """n feature rows of candidates on a synthetic genome, labels 1.4 + 2.2 (logistic - 0.5) + noise.  dup_frac: that share of rows repeats an
    earlier row with a label of its own (exact ties in working-set selection); zero_rows: rows set to all zeros."""
    R = po.refdrv()
    rng = np.random.default_rng(seed)
    g = synth.random_genome(40000, seed)
    X, Y = [], []
    while len(X) < n:
        e = int(rng.integers(16, 31)); l = int(rng.integers(18, 31)); ss = int(rng.integers(75, 215))
        p = int(rng.integers(400, len(g) - 700)); strand = int(rng.integers(0, 2))
        ext = g[p - 1 - e:p - 1] if strand == 0 else g[p - 1 + ss:p - 1 + ss + e]
        ins = g[p - 1:p - 1 + ss]
        lig = g[p - 1 + ss:p - 1 + ss + l] if strand == 0 else g[p - 1 - l:p - 1]
        ec = int(rng.choice([1, 1, 1, 1, 2, 3, 7, 20])); lc = int(rng.choice([1, 1, 1, 1, 2, 5, 19]))
        lrc = rng.uniform(0, 0.3, 44)
        x = np.empty(192)
        R.ref_parameters(strand, ext, lig, ins, ec, lc, MIDDLE, lrc.ctypes.data_as(_dp), x.ctypes.data_as(_dp))
        if not np.all(np.isfinite(x)) or not np.any(x):
            continue
        s = R.ref_logistic(strand, ext, lig, ins, ec, lc, MIDDLE)
        X.append(x); Y.append(1.4 + 2.2 * (s - 0.5) + 0.08 * rng.standard_normal())
    X = np.array(X); Y = np.array(Y)
    if dup_frac > 0:
        k = int(dup_frac * n)
        dst = rng.choice(np.arange(n // 2, n), size=k, replace=False)
        src = rng.integers(0, n // 2, size=k)
        X[dst] = X[src]
        Y[dst] = Y[src] + 0.3 * rng.standard_normal(k)
    if zero_rows:
        X[rng.choice(n, size=zero_rows, replace=False)] = 0.0
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def ref_model(X, Y, gamma, C_, p, path):
    nsv = po.refdrv().ref_svm_train_save(X.shape[0], X.ctypes.data_as(_dp), Y.ctypes.data_as(_dp), gamma, C_, p, path.encode())
    assert nsv >= 0
    return open(path, "rb").read()


def write_libsvm(path, X, Y):
    with open(path, "w") as fh:
        for x, y in zip(X, Y):
            fh.write(repr(float(y)) + "".join(f" {j + 1}:{float(v)!r}" for j, v in enumerate(x) if v != 0.0) + "\n")


def new_accel():
    P = capi.make_params(130, 140, score_method=capi.SCORE_SVR, arm_pairs=synth.arm_pairs_from_sums([43, 44, 45]))
    return capi.Accel(P, device=0), P


def first_diff(a: bytes, b: bytes) -> str:
    la, lb = a.split(b"\n"), b.split(b"\n")
    i = next((k for k, (u, v) in enumerate(zip(la, lb)) if u != v), min(len(la), len(lb)))
    return f"line {i + 1}: ours {la[i][:200] if i < len(la) else None!r} ref {lb[i][:200] if i < len(lb) else None!r}"


CASES = {
    "fixture_recipe_360": dict(n=360, seed=4242, gamma=2e-4, C=8.0, p=0.12),
    "n1500_default": dict(n=1500, seed=7, gamma=1 / 192, C=1.0, p=0.1),
    "n4000_wide": dict(n=4000, seed=11, gamma=0.05, C=32.0, p=0.05),
    "duplicated_rows": dict(n=1200, seed=13, gamma=0.01, C=4.0, p=0.05, dup_frac=0.1),
    "zero_rows": dict(n=800, seed=17, gamma=0.02, C=2.0, p=0.1, zero_rows=12),
    # the edges: fewer rows than a wavefront or a Gram tile, no support vector at all, every support vector at the bound, K = 1 everywhere
    "n1": dict(n=1, seed=31, gamma=0.01, C=4.0, p=0.05),
    "n2": dict(n=2, seed=32, gamma=0.01, C=4.0, p=0.001),
    "n17": dict(n=17, seed=33, gamma=0.01, C=4.0, p=0.05),
    "no_sv": dict(n=300, seed=37, gamma=0.01, C=4.0, p=10.0),              # p above the spread of the labels
    "all_bounded": dict(n=300, seed=41, gamma=0.01, C=1e-3, p=0.05),
    "gamma0": dict(n=300, seed=43, gamma=0.0, C=4.0, p=0.05),
}


@need_ref
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_file_is_libsvms_byte_for_byte(name, tmp_path):
    c = CASES[name]
    X, Y = training_set(c["n"], c["seed"], c.get("dup_frac", 0.0), c.get("zero_rows", 0))
    want = ref_model(X, Y, c["gamma"], c["C"], c["p"], str(tmp_path / "ref.model"))
    acc, _ = new_accel()
    info = acc.train_svr(X, Y, c["gamma"], c["C"], c["p"], model_path=str(tmp_path / "ours.model"))
    got = open(tmp_path / "ours.model", "rb").read()
    assert got == want, f"{name}: {first_diff(got, want)}; info {info}"
    n_sv, gamma, _ = acc.model_info()
    assert n_sv == info["n_sv"] == int(want.split(b"total_sv ")[1].split(b"\n")[0]) and gamma == float("%g" % c["gamma"])
    if name == "no_sv":
        assert info["n_sv"] == 0 and b"total_sv 0\n" in want
    if name == "all_bounded":
        assert info["n_bsv"] == info["n_sv"] > 0, info
    if name == "n4000_wide":                                 # the shrinking path: do_shrinking, its unshrink and the final reconstruct_gradient
        assert info["n_shrink"] > 0 and info["n_reconstruct"] > 0, info
    acc.close()


@need_ref
def test_training_twice_gives_the_same_bytes(tmp_path):
    X, Y = training_set(1500, 7)
    acc, _ = new_accel()
    acc.train_svr(X, Y, 1 / 192, 1.0, 0.1, model_path=str(tmp_path / "a.model"))
    acc.train_svr(X, Y, 1 / 192, 1.0, 0.1, model_path=str(tmp_path / "b.model"))
    assert open(tmp_path / "a.model", "rb").read() == open(tmp_path / "b.model", "rb").read()
    acc.close()


@need_ref
def test_trained_handle_scores_as_the_loaded_file(tmp_path):
    """After train_svr the handle scores exactly as a fresh handle that loaded the written file, and within 1e-5 of the reference's svm_predict."""
    X, Y = training_set(800, 23)
    path = str(tmp_path / "m.model")
    acc, P = new_accel()
    acc.train_svr(X, Y, 0.01, 4.0, 0.05, model_path=path)
    fresh, _ = new_accel()
    fresh.load_model_file(path)
    genome = synth.random_genome(12000, 5, n_run_frac=0.002, n_run_len=6)
    regions = [capi.build_region(genome, "1", 5000, 5055, P, bwa_mode="hashed", label="s1", lrc=np.linspace(0.01, 0.3, 44)),
               capi.build_region(genome, "1", 7000, 7090, P, bwa_mode="hashed", label="s2", lrc=np.linspace(0.3, 0.01, 44))]
    ga, sa, ra = acc.score_regions(regions, capi.SCORE_SVR)
    gb, sb, rb = fresh.score_regions(regions, capi.SCORE_SVR)
    assert np.array_equal(ra, rb)
    assert np.array_equal(sa, sb, equal_nan=True)
    # a sample of valid candidates through the literal kernel: features and scores against the reference's prediction from the file
    acc.upload(regions)
    rng = np.random.default_rng(3)
    cands = []
    for ri, g in enumerate(ga):
        rec = ra[g.offset:g.offset + g.count]
        valid = np.nonzero((capi.rec_flags(rec) & capi.FLAG_VALID) != 0)[0]
        for idx in rng.choice(valid, size=min(40, len(valid)), replace=False):
            A = P.n_arm_pairs
            a = int(idx % A); row = int(idx // A); st = row & 1; rest = row >> 1
            ki, pi = rest % g.n_sizes, rest // g.n_sizes
            cands.append((ri, g.first_pos + pi, P.max_capture_size - (g.first_size_index + ki) * P.capture_increment, P.arm_ext[a], P.arm_lig[a], st))
    assert len(cands) > 20
    s_a, _, feats, _ = acc.score_candidates(cands, capi.SCORE_SVR, want_features=True)
    fresh.upload(regions)
    s_b = fresh.score_candidates(cands, capi.SCORE_SVR)[0]
    assert np.array_equal(s_a, s_b, equal_nan=True)
    R = po.refdrv()
    m = R.ref_svm_load_model(path.encode())
    try:
        for s, x in zip(s_a, feats):
            x = np.ascontiguousarray(x)
            want = R.ref_predict_text(m, x.ctypes.data_as(_dp), 192)
            assert (np.isnan(s) and np.isnan(want)) or abs(s - want) <= 1e-5, (s, want)
    finally:
        R.ref_svm_free_model(m)
    acc.close(); fresh.close()


def outcome(call):
    """what a call gives: its result, or the text of its refusal"""
    try:
        return "ok", call()
    except capi.AccelError as e:
        return "refused", str(e)


def same_outcome(a, b):
    if a[0] != b[0]:
        return False
    if a[0] == "refused":
        return a[1] == b[1]
    return all((u is None and v is None) or np.array_equal(u, v, equal_nan=u.dtype.kind == "f") for u, v in zip(a[1], b[1]))


@need_ref
def test_trained_handle_without_support_vectors_behaves_as_the_loaded_file(tmp_path):
    """The no_sv case leaves a model of zero support vectors: the handle that trained it and a fresh handle that loads the file give the same scores, or
    the same refusal, for the regions and for a list of 200 candidates."""
    c = CASES["no_sv"]
    X, Y = training_set(c["n"], c["seed"])
    path = str(tmp_path / "m.model")
    acc, P = new_accel()
    info = acc.train_svr(X, Y, c["gamma"], c["C"], c["p"], model_path=path)
    assert info["n_sv"] == 0 and b"total_sv 0\n" in open(path, "rb").read()
    fresh, _ = new_accel()
    fresh.load_model_file(path)
    assert acc.model_info() == fresh.model_info() and acc.model_info()[0] == 0
    genome = synth.random_genome(12000, 5, n_run_frac=0.002, n_run_len=6)
    regions = [capi.build_region(genome, "1", 5000, 5055, P, bwa_mode="hashed", label="s1", lrc=np.linspace(0.01, 0.3, 44)),
               capi.build_region(genome, "1", 7000, 7090, P, bwa_mode="hashed", label="s2", lrc=np.linspace(0.3, 0.01, 44))]
    ra = outcome(lambda: acc.score_regions(regions, capi.SCORE_SVR)[1:])
    rb = outcome(lambda: fresh.score_regions(regions, capi.SCORE_SVR)[1:])
    assert same_outcome(ra, rb), (ra, rb)
    # 200 valid candidates, found by the logistic pass (it needs no model)
    grids, _, rec = acc.score_regions(regions, capi.SCORE_LOGISTIC)
    rng = np.random.default_rng(3)
    cands = []
    for ri, g in enumerate(grids):
        valid = np.nonzero((capi.rec_flags(rec[g.offset:g.offset + g.count]) & capi.FLAG_VALID) != 0)[0]
        for idx in rng.choice(valid, size=min(100, len(valid)), replace=False):
            A = P.n_arm_pairs
            a = int(idx % A); row = int(idx // A); st = row & 1; rest = row >> 1
            ki, pi = rest % g.n_sizes, rest // g.n_sizes
            cands.append((ri, g.first_pos + pi, P.max_capture_size - (g.first_size_index + ki) * P.capture_increment, P.arm_ext[a], P.arm_lig[a], st))
    assert len(cands) == 200
    acc.upload(regions); fresh.upload(regions)
    ca = outcome(lambda: acc.score_candidates(cands, capi.SCORE_SVR)[:2])
    cb = outcome(lambda: fresh.score_candidates(cands, capi.SCORE_SVR)[:2])
    assert same_outcome(ca, cb), (ca, cb)
    acc.close(); fresh.close()


def test_invalid_arguments_leave_the_model_alone(tmp_path):
    acc, _ = new_accel()
    model = os.path.join(H.GOLDEN, "models", "svr_libsvm_trained.model")
    acc.load_model_file(model)
    before = acc.model_info()
    rng = np.random.default_rng(1)
    X = rng.uniform(0, 1, (50, 192)); Y = rng.uniform(0, 3, 50)
    out = str(tmp_path / "never.model")
    bad_x = X.copy(); bad_x[7, 3] = -np.inf
    bad_y = Y.copy(); bad_y[2] = np.nan
    cases = [dict(cost=0.0), dict(cost=-1.0), dict(epsilon_p=-0.1), dict(eps=0.0), dict(gamma=-1.0), dict(shrinking=0),
             dict(x=bad_x), dict(y=bad_y), dict(x=X[:0], y=Y[:0])]
    for c in cases:
        kw = dict(x=X, y=Y, gamma=0.01, cost=1.0, epsilon_p=0.1, eps=1e-3, shrinking=1)
        kw.update(c)
        with pytest.raises(capi.AccelError, match=r"error -1: \S") as ei:
            acc.train_svr(kw["x"], kw["y"], kw["gamma"], kw["cost"], kw["epsilon_p"], kw["eps"], model_path=out, shrinking=kw["shrinking"])
        assert acc.model_info() == before, (c, str(ei.value))
        assert not os.path.exists(out)
    # past the kernel-matrix budget: refused before any allocation
    n = 131072 + 1                                          # MIPGEN_SVR_TRAIN_MAX_ROWS + 1
    big = np.zeros((n, 192)); yb = np.zeros(n)
    with pytest.raises(capi.AccelError, match=r"error -5: \S"):
        acc.train_svr(big, yb, 0.01, 1.0, 0.1, model_path=out)
    assert acc.model_info() == before and not os.path.exists(out)
    acc.close()


@need_ref
def test_cli_writes_libsvms_model_file(tmp_path):
    c = CASES["duplicated_rows"]
    X, Y = training_set(c["n"], c["seed"], c["dup_frac"])
    write_libsvm(str(tmp_path / "train.txt"), X, Y)
    want = ref_model(X, Y, c["gamma"], c["C"], c["p"], str(tmp_path / "ref.model"))
    p = subprocess.run([TRAIN_BIN, "-s", "3", "-t", "2", "-g", repr(c["gamma"]), "-c", repr(c["C"]), "-p", repr(c["p"]), "-q", "train.txt"],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    got = open(tmp_path / "train.txt.model", "rb").read()
    assert got == want, first_diff(got, want)


@need_ref
@pytest.mark.skipif(not rr.have_reference(), reason="reference binary (oracle/_ref) not built")
def test_cli_trained_model_designs_as_the_reference(tmp_path):
    """mipgen_svr_train writes mipgen_svr.model; `mipgen -score_method svr` with it writes the files the reference binary writes with it."""
    meta = H.load_design("svr_small")
    X, Y = training_set(600, 29)
    work = tmp_path / "ours"
    argv = H.prepare_cli_workdir(meta, str(work))
    write_libsvm(str(tmp_path / "train.txt"), X, Y)
    p = subprocess.run([TRAIN_BIN, "-g", "0.01", "-c", "4", "-p", "0.05", "-q", str(tmp_path / "train.txt"), str(work / "mipgen_svr.model")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    want = ref_model(X, Y, 0.01, 4.0, 0.05, str(tmp_path / "ref.model"))
    assert open(work / "mipgen_svr.model", "rb").read() == want
    env = dict(os.environ, FAKEBWA_MODE=meta["bwa"])
    q = subprocess.run(argv, cwd=work, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert q.returncode == 0, q.stderr.decode()[-3000:]
    rwork = tmp_path / "ref"
    shutil.copytree(work / "genome", rwork / "genome")
    shutil.copy(work / "regions.bed", rwork / "regions.bed")
    r = rr.run_reference(str(rwork), str(rwork / "genome"), str(rwork / "regions.bed"), "out", meta["minC"], meta["maxC"], score_method="svr",
                         model_path=str(work / "mipgen_svr.model"), bwa_mode=meta["bwa"],
                         extra=["-feature_flank", str(meta["flank"]), "-tag_sizes", meta["tags"], "-arm_length_sums", ",".join(map(str, meta["sums"]))],
                         timeout=900)
    assert r["returncode"] == 0, r["stderr"][-3000:]
    for key in ("collapsed_mips", "picked_mips", "snp_mips"):
        got = open(work / f"out.{key}.txt", "rb").read()
        ref = open(r[key], "rb").read()
        assert got == ref, (key, first_diff(got, ref))
    got_all = open(work / "out.all_mips.txt", "rb").read()
    ref_all = H.normalise_all_mips(open(r["all_mips"], "rb").read())
    assert got_all.count(b"\n") > 100
    assert got_all == ref_all, first_diff(got_all, ref_all)
