"""GPU: mipgen_accel_cross_validate_svr / `mipgen_svr_cv`, libsvm's svm_cross_validation for a grid of parameter sets with every (set, fold)
solved as one batch on the device, against the reference's own code: every fold model against svm_train + svm_save_model on the fold's rows
(oracle ref_svm_train_save) byte for byte, the held-out predictions against svm_cross_validation (called through ctypes on the reference
driver, libc's srand(seed) first) within 1e-5 on every row - the project's gate for SVR scores against svm_predict.

Every device step runs in a child process under a timeout of its own (`python -m tests.test_gpu_svr_cv job.pkl`: a list of operations on one
handle, results pickled back), so a device fault ends that step and nothing else is started on the device by that test.

Measured on one MI355X (printed by test_fold_models_and_targets_are_libsvms and test_grid_is_its_points): the largest |target - svm_predict|
over the 4,630 rows of the seven checked points is 3.6e-15 (n 1,200 with duplicated rows; 0 to 1.8e-15 elsewhere): rounding of a sum of
a few hundred terms of size ~1, where glibc's exp and the correctly rounded one differ in the last bit now and then."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from mipgen_amd import capi
from oracle import pyoracle as po
from tests.test_gpu_svr_train import first_diff, new_accel, ref_model, training_set, write_libsvm

pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(not po.have_refdrv(), reason="reference driver (oracle/_ref) not built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CV_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_svr_cv")
GATE = 1e-5                                     # DESIGN.md §2 "Gates": SVR scores against svm_predict


# ---- the child: operations on one handle ---------------------------------------------------------------------------------------------------
def _child(job_path: str) -> None:
    job = pickle.load(open(job_path, "rb"))
    acc, _ = new_accel()
    if job.get("model"):
        acc.load_model_file(job["model"])
    out = []
    for op in job["ops"]:
        kind = op["op"]
        if kind == "cv":
            x, y = op.get("x", job.get("x")), op.get("y", job.get("y"))
            if "zero_rows" in op:                               # too large to pickle: built here
                x, y = np.zeros((op["zero_rows"], 192)), np.zeros(op["zero_rows"])
            try:
                target, res = acc.cross_validate_svr(x, y, op["points"], nr_fold=op["folds"],
                                                     seed=op.get("seed", 1), eps=op.get("eps", 1e-3), fold_model_prefix=op.get("prefix"))
                out.append(dict(target=target, results=res))
            except capi.AccelError as e:
                out.append(dict(error=str(e)))
        elif kind == "train":
            out.append(acc.train_svr(job["x"], job["y"], op["gamma"], op["C"], op["p"], model_path=op["path"]))
        elif kind == "model_info":
            out.append(acc.model_info())
    acc.close()
    pickle.dump(out, open(job_path + ".out", "wb"))


def run_ops(tmp_path, ops, x=None, y=None, model=None, timeout=900):
    job = str(tmp_path / "job.pkl")
    pickle.dump(dict(ops=ops, x=x, y=y, model=model), open(job, "wb"))
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_svr_cv", job], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, f"device step ended with status {p.returncode}: {p.stderr.decode()[-3000:]}"
    return pickle.load(open(job + ".out", "rb"))


# ---- the oracle: svm_cross_validation of the reference, through ctypes (svm.h:12-47) -----------------------------------------------------------
class SvmNode(C.Structure):
    _fields_ = [("index", C.c_int), ("value", C.c_double)]


class SvmProblem(C.Structure):
    _fields_ = [("l", C.c_int), ("y", C.POINTER(C.c_double)), ("x", C.POINTER(C.POINTER(SvmNode)))]


class SvmParameter(C.Structure):
    _fields_ = [("svm_type", C.c_int), ("kernel_type", C.c_int), ("degree", C.c_int), ("gamma", C.c_double), ("coef0", C.c_double),
                ("cache_size", C.c_double), ("eps", C.c_double), ("C", C.c_double), ("nr_weight", C.c_int), ("weight_label", C.POINTER(C.c_int)),
                ("weight", C.POINTER(C.c_double)), ("nu", C.c_double), ("p", C.c_double), ("shrinking", C.c_int), ("probability", C.c_int)]


_PRINT = C.CFUNCTYPE(None, C.c_char_p)(lambda s: None)


def ref_cross_validation(X, Y, gamma, C_, p, folds, seed, eps=1e-3):
    """target of svm_cross_validation(prob, param, folds) after srand(seed); rows hold their non-zero features, as ref_svm_train_save's do."""
    R = po.refdrv()
    n = X.shape[0]
    nodes = []
    first = []
    for row in X:
        first.append(len(nodes))
        nodes.extend((j + 1, float(v)) for j, v in enumerate(row) if v != 0.0)
        nodes.append((-1, 0.0))
    pool = (SvmNode * len(nodes))(*nodes)
    xs = (C.POINTER(SvmNode) * n)(*[C.cast(C.byref(pool, f * C.sizeof(SvmNode)), C.POINTER(SvmNode)) for f in first])
    ys = (C.c_double * n)(*[float(v) for v in Y])
    prob = SvmProblem(n, ys, xs)
    par = SvmParameter(svm_type=3, kernel_type=2, degree=3, gamma=gamma, coef0=0.0, cache_size=100.0, eps=eps, C=C_, nr_weight=0, nu=0.5, p=p,
                       shrinking=1, probability=0)
    R.svm_set_print_string_function.argtypes = [C.c_void_p]
    R.svm_set_print_string_function.restype = None
    R.svm_set_print_string_function(C.cast(_PRINT, C.c_void_p))
    R.svm_cross_validation.argtypes = [C.POINTER(SvmProblem), C.POINTER(SvmParameter), C.c_int, C.POINTER(C.c_double)]
    R.svm_cross_validation.restype = None
    target = (C.c_double * n)()
    libc = C.CDLL("libc.so.6")
    libc.srand.argtypes = [C.c_uint]
    libc.srand(seed)
    R.svm_cross_validation(C.byref(prob), C.byref(par), folds, target)
    return np.array(target[:])


def cv_sums(target, Y):
    """svm-train's do_cross_validation: mse and r2 over target and y in row order, in Python floats"""
    n = len(Y)
    te = sv = sy = svv = syy = svy = 0.0
    for v, y in zip(map(float, target), map(float, Y)):
        te += (v - y) * (v - y)
        sv += v; sy += y; svv += v * v; syy += y * y; svy += v * y
    return te / n, ((n * svy - sv * sy) * (n * svy - sv * sy)) / ((n * svv - sv * sv) * (n * syy - sy * sy))


def check_point_against_oracle(tmp_path, X, Y, point, folds, seed, prefix, q, target, result, tag):
    """items 5 and 6 for one point: fold models byte for byte, targets within the gate on every row, mse / r2 bit for bit over the returned target"""
    gamma, C_, p = point
    n = X.shape[0]
    perm, start = capi.svr_cv_folds(n, folds, seed)
    n_sv = 0
    for f in range(len(start) - 1):
        rows = np.concatenate([perm[:start[f]], perm[start[f + 1]:]])
        want = ref_model(np.ascontiguousarray(X[rows]), np.ascontiguousarray(Y[rows]), gamma, C_, p, str(tmp_path / "ref_fold.model"))
        got = open(f"{prefix}.{q}.{f}.model", "rb").read()
        assert got == want, f"{tag} point {q} fold {f}: {first_diff(got, want)}"
        n_sv += int(want.split(b"total_sv ")[1].split(b"\n")[0])
    assert result["n_sv_total"] == n_sv and result["iterations"] > 0
    want_t = ref_cross_validation(X, Y, gamma, C_, p, folds, seed)
    assert target.shape == (n,) and np.all(np.isfinite(target))
    diff = np.abs(target - want_t)
    print(f"{tag} point {q}: n {n} folds {len(start) - 1} max |target - svm_cross_validation| = {diff.max():.3e} (row {int(diff.argmax())}), "
          f"mse {result['mse']!r} r2 {result['r2']!r} iterations {result['iterations']} nSV {n_sv}")
    assert np.all(diff <= GATE), f"{tag} point {q}: {int((diff > GATE).sum())} rows beyond {GATE}, max {diff.max()}"
    mse, r2 = cv_sums(target, Y)
    assert result["mse"] == mse and result["r2"] == r2, (result, mse, r2)


CASES = {
    "n600_5fold": dict(n=600, seed=31, folds=5, cv_seed=1, point=(0.01, 4.0, 0.05)),
    "n1200_dup_3fold": dict(n=1200, seed=13, dup_frac=0.1, folds=3, cv_seed=1, point=(0.01, 4.0, 0.05)),
    "n400_10fold": dict(n=400, seed=37, folds=10, cv_seed=7, point=(1 / 192, 1.0, 0.1)),
    "n30_leave_one_out": dict(n=30, seed=41, folds=50, cv_seed=1, point=(0.02, 2.0, 0.1)),
}


@need_ref
@pytest.mark.parametrize("name", sorted(CASES))
def test_fold_models_and_targets_are_libsvms(name, tmp_path):
    c = CASES[name]
    X, Y = training_set(c["n"], c["seed"], c.get("dup_frac", 0.0))
    prefix = str(tmp_path / "fold")
    (r,) = run_ops(tmp_path, [dict(op="cv", points=[c["point"]], folds=c["folds"], seed=c["cv_seed"], prefix=prefix)], X, Y)
    assert "error" not in r, r
    assert len([f for f in os.listdir(tmp_path) if f.startswith("fold.0.")]) == min(c["folds"], c["n"])
    check_point_against_oracle(tmp_path, X, Y, c["point"], c["folds"], c["cv_seed"], prefix, 0, r["target"][0], r["results"][0], name)


@need_ref
def test_grid_is_its_points(tmp_path):
    """3 gammas x 3 C x 2 p x 5 folds at n = 800 - 90 solves in one call - against 18 one-point calls: the same target bits, the same fold-model
    bytes; three of the points against the oracle; another seed gives other folds."""
    X, Y = training_set(800, 43)
    points = [(g, c_, p) for g in (0.005, 0.01, 0.02) for c_ in (1.0, 4.0, 16.0) for p in (0.05, 0.1)]
    ops = [dict(op="cv", points=points, folds=5, seed=1, prefix=str(tmp_path / "grid"))]
    ops += [dict(op="cv", points=[pt], folds=5, seed=1, prefix=str(tmp_path / f"one{q}")) for q, pt in enumerate(points)]
    ops += [dict(op="cv", points=points[:2], folds=5, seed=7)]
    out = run_ops(tmp_path, ops, X, Y, timeout=1200)
    assert all("error" not in r for r in out), out
    grid = out[0]
    assert grid["target"].shape == (18, 800)
    for q in range(18):
        one = out[1 + q]
        assert np.array_equal(grid["target"][q].view(np.uint64), one["target"][0].view(np.uint64)), f"point {q}: target bits differ"
        assert grid["results"][q] == one["results"][0], (q, grid["results"][q], one["results"][0])
        for f in range(5):
            a = open(tmp_path / f"grid.{q}.{f}.model", "rb").read()
            b = open(tmp_path / f"one{q}.0.{f}.model", "rb").read()
            assert a == b, f"point {q} fold {f}: {first_diff(a, b)}"
    for q in (0, 7, 17):
        check_point_against_oracle(tmp_path, X, Y, points[q], 5, 1, str(tmp_path / "grid"), q, grid["target"][q], grid["results"][q], "grid")
    other = out[19]
    assert not np.array_equal(other["target"][0], grid["target"][0]) and not np.array_equal(other["target"][1], grid["target"][1])
    assert not np.array_equal(capi.svr_cv_folds(800, 5, 1)[0], capi.svr_cv_folds(800, 5, 7)[0])


@need_ref
def test_training_around_a_cross_validation_is_unchanged(tmp_path):
    """train_svr before and after a cross-validation on the same handle writes the same bytes - libsvm's - and CV leaves the handle's model alone"""
    X, Y = training_set(700, 47)
    a, b = str(tmp_path / "a.model"), str(tmp_path / "b.model")
    ops = [dict(op="train", gamma=0.01, C=4.0, p=0.05, path=a), dict(op="model_info"),
           dict(op="cv", points=[(0.02, 1.0, 0.1), (0.005, 8.0, 0.1)], folds=4, seed=3), dict(op="model_info"),
           dict(op="train", gamma=0.01, C=4.0, p=0.05, path=b)]
    out = run_ops(tmp_path, ops, X, Y)
    assert "error" not in out[2], out[2]
    assert out[1] == out[3] and out[1][0] == out[0]["n_sv"]
    assert open(a, "rb").read() == open(b, "rb").read() == ref_model(X, Y, 0.01, 4.0, 0.05, str(tmp_path / "ref.model"))
    for k in ("iterations", "n_sv", "n_bsv", "rho", "obj", "n_shrink", "n_reconstruct"):
        assert out[0][k] == out[4][k], k


@need_ref
def test_cli_prints_svm_trains_lines_and_writes_the_best_model(tmp_path):
    X, Y = training_set(500, 53)
    write_libsvm(str(tmp_path / "train.txt"), X, Y)
    gammas, costs = (0.005, 0.02), (1.0, 8.0)
    points = [(g, c_, 0.1) for g in gammas for c_ in costs]
    out = run_ops(tmp_path, [dict(op="cv", points=[(0.01, 4.0, 0.05)], folds=5, seed=1), dict(op="cv", points=points, folds=4, seed=5)], X, Y)
    one, grid = out[0]["results"][0], out[1]["results"]
    p = subprocess.run([CV_BIN, "-g", "0.01", "-c", "4", "-p", "0.05", "train.txt"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    assert lines == ["gamma=0.01 C=4 p=0.05 mse=%g r2=%g" % (one["mse"], one["r2"]),
                     "Cross Validation Mean squared error = %g" % one["mse"],
                     "Cross Validation Squared correlation coefficient = %g" % one["r2"],
                     "best gamma=0.01 C=4 p=0.05 mse=%g" % one["mse"]], lines
    want_t = ref_cross_validation(X, Y, 0.01, 4.0, 0.05, 5, 1)
    assert np.all(np.abs(out[0]["target"][0] - want_t) <= GATE)
    p = subprocess.run([CV_BIN, "-v", "4", "-seed", "5", "-g", "0.005,0.02", "-c", "1,8", "-o", "best.model", "train.txt"], cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    best = min(range(4), key=lambda q: (grid[q]["mse"], q))
    assert lines[:4] == ["gamma=%g C=%g p=%g mse=%g r2=%g" % (*points[q], grid[q]["mse"], grid[q]["r2"]) for q in range(4)], lines
    assert lines[4:] == ["best gamma=%g C=%g p=%g mse=%g" % (*points[best], grid[best]["mse"])], lines
    assert len({r["mse"] for r in grid}) == 4                        # the choice is a real one
    want = ref_model(X, Y, points[best][0], points[best][1], points[best][2], str(tmp_path / "ref.model"))
    got = open(tmp_path / "best.model", "rb").read()
    assert got == want, first_diff(got, want)


def test_invalid_arguments_leave_the_handle_usable(tmp_path):
    from tests import helpers as H
    rng = np.random.default_rng(1)
    X = rng.uniform(0, 1, (60, 192)); Y = rng.uniform(0, 3, 60)
    bad_x = X.copy(); bad_x[7, 3] = np.nan
    bad_y = Y.copy(); bad_y[2] = np.inf
    ok = (0.01, 1.0, 0.1)
    n_big = 131072 + 1                                          # MIPGEN_SVR_TRAIN_MAX_ROWS + 1
    bad = [dict(points=[ok], folds=1), dict(points=[ok], folds=0), dict(points=[], folds=5), dict(points=[ok, (-1.0, 1.0, 0.1)], folds=5),
           dict(points=[(0.01, 0.0, 0.1)], folds=5), dict(points=[(0.01, 1.0, -0.1)], folds=5), dict(points=[(float("nan"), 1.0, 0.1)], folds=5),
           dict(points=[ok], folds=5, eps=0.0), dict(points=[ok], folds=5, x=bad_x), dict(points=[ok], folds=5, y=bad_y),
           dict(points=[ok], folds=5, x=X[:1], y=Y[:1]), dict(points=[ok], folds=5, x=X[:0], y=Y[:0])]
    ops = [dict(op="model_info")] + [dict(op="cv", **b) for b in bad]
    ops += [dict(op="cv", points=[ok], folds=5, zero_rows=n_big), dict(op="model_info"),
            dict(op="cv", points=[ok], folds=5), dict(op="model_info")]
    out = run_ops(tmp_path, ops, X, Y, model=os.path.join(H.GOLDEN, "models", "svr_libsvm_trained.model"))
    for b, r in zip(bad, out[1:1 + len(bad)]):
        assert "error" in r and r["error"].startswith("mipgen_accel error -1: ") and len(r["error"]) > 25, (b, r)
    assert out[1 + len(bad)]["error"].startswith("mipgen_accel error -5: "), out[1 + len(bad)]
    assert out[0] == out[2 + len(bad)] == out[4 + len(bad)]
    good = out[3 + len(bad)]
    assert "error" not in good and np.all(np.isfinite(good["target"])) and good["results"][0]["mse"] == cv_sums(good["target"][0], Y)[0]


if __name__ == "__main__":
    _child(sys.argv[1])
