#!/usr/bin/env python3
"""Rate of SVR cross-validation on the device (mipgen_accel_cross_validate_svr: every fold one workgroup of one batch) against the same folds
solved one after the other, on feature rows of real candidates (tests/test_gpu_svr_train.py's training_set).  One JSON line per size; every leg
after a warm-up call and run twice (both times are printed: their spread is the noise any ratio has to beat):

  a  one cross_validate_svr call (folds solved together, plus the held-out predictions)
  b  the fold sub-problems through sequential train_svr calls - only entry points that predate cross-validation, so this leg also runs on an
     older checkout (there `a` and `d` are skipped) and gives the baseline
  c  svm_cross_validation of the reference's libsvm on one CPU core (--ref-max-n: sizes above it are skipped)
  d  (--grid-n, default 8000) an 18-point grid of ONE gamma, 6 C x 3 p: 90 problems over one matrix, all live at once, against 18 x a

    python tools/svr_cv_rate.py [--sizes 2000,8000,20000] [--folds 5] [--ref-max-n 8000] [--grid-n 8000] [--legs abcd]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mipgen_amd import capi, synth  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests.test_gpu_svr_train import training_set  # noqa: E402

HAVE_CV = hasattr(capi.Accel, "cross_validate_svr")


def libsvm_folds(n, folds, seed=1):
    """svm.cpp:2408-2415 on libc's generator (a checkout without capi.svr_cv_folds has to make the same folds)"""
    import ctypes as C
    libc = C.CDLL("libc.so.6")
    libc.srand.argtypes = [C.c_uint]
    libc.srand(seed)
    perm = list(range(n))
    for i in range(n):
        j = i + libc.rand() % (n - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm), [i * n // folds for i in range(folds + 1)]


def twice(fn):
    out = []
    for _ in range(2):
        t0 = time.perf_counter()
        r = fn()
        out.append(round(time.perf_counter() - t0, 4))
    return out, r


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,8000,20000")
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--gamma", type=float, default=1 / 192)
    ap.add_argument("--cost", type=float, default=8.0)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=101)
    ap.add_argument("--ref-max-n", type=int, default=8000, help="largest size the libsvm leg runs at")
    ap.add_argument("--grid-n", type=int, default=8000, help="size at which the 18-point grid leg runs (0: never)")
    ap.add_argument("--legs", default="abcd")
    a = ap.parse_args()
    P = capi.make_params(130, 140, score_method=capi.SCORE_SVR, arm_pairs=synth.arm_pairs_from_sums([43, 44, 45]))
    acc = capi.Accel(P, device=0)
    pt = (a.gamma, a.cost, a.p)
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "m.model")
        Xw, Yw = training_set(300, a.seed)                                  # warm-up: the first launches load the code objects
        acc.train_svr(Xw, Yw, a.gamma, a.cost, a.p, model_path=model)
        if HAVE_CV:
            acc.cross_validate_svr(Xw, Yw, [pt], nr_fold=a.folds)
        for n in (int(s) for s in a.sizes.split(",")):
            X, Y = training_set(n, a.seed + n)
            row = {"n": n, "folds": a.folds, "gamma": a.gamma, "C": a.cost, "p": a.p}
            if HAVE_CV and "a" in a.legs:
                ts, (_, res) = twice(lambda: acc.cross_validate_svr(X, Y, [pt], nr_fold=a.folds))
                row.update(a_cv_call_s=ts, a_iterations=res[0]["iterations"], a_mse=res[0]["mse"])
            if "b" in a.legs:
                perm, start = libsvm_folds(n, a.folds)
                subs = []
                for f in range(a.folds):
                    rows = np.concatenate([perm[:start[f]], perm[start[f + 1]:]])
                    subs.append((np.ascontiguousarray(X[rows]), np.ascontiguousarray(Y[rows])))
                ts, infos = twice(lambda: [acc.train_svr(xs, ys, a.gamma, a.cost, a.p, model_path=model) for xs, ys in subs])
                slow = max(infos, key=lambda i: i["solve_ms"])
                row.update(b_sequential_s=ts, b_iterations=sum(i["iterations"] for i in infos), b_solve_ms=[round(i["solve_ms"], 1) for i in infos],
                           b_slowest_us_per_iter=round(1e3 * slow["solve_ms"] / max(slow["iterations"], 1), 2), b_slowest_iterations=slow["iterations"])
                if "a_cv_call_s" in row:
                    row["a_over_b"] = round(min(row["a_cv_call_s"]) / min(ts), 3)
                    # the batch ends with its slowest problem: its wall time over that problem's iteration count
                    row["a_us_per_iter_of_slowest"] = round(1e6 * min(row["a_cv_call_s"]) / max(slow["iterations"], 1), 2)
            if "c" in a.legs and po.have_refdrv() and n <= a.ref_max_n:
                from tests.test_gpu_svr_cv import ref_cross_validation
                t0 = time.perf_counter()
                ref_cross_validation(X, Y, a.gamma, a.cost, a.p, a.folds, 1)
                row["c_libsvm_s"] = round(time.perf_counter() - t0, 3)
                if "a_cv_call_s" in row:
                    row["a_over_c"] = round(min(row["a_cv_call_s"]) / row["c_libsvm_s"], 4)
            elif "c" in a.legs:
                row["c_libsvm_s"] = None                                   # skipped: above --ref-max-n (or no reference driver)
            if HAVE_CV and "d" in a.legs and n == a.grid_n:
                grid = [(a.gamma, c_, p) for c_ in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0) for p in (0.05, 0.1, 0.2)]
                ts, (_, res) = twice(lambda: acc.cross_validate_svr(X, Y, grid, nr_fold=a.folds))
                slow_it = max(r["iterations"] for r in res)
                row.update(d_grid18_s=ts, d_problems=len(grid) * a.folds, d_iterations=sum(r["iterations"] for r in res), d_most_iterations_of_a_point=slow_it)
                if "a_cv_call_s" in row:
                    row["d_over_a"] = round(min(ts) / min(row["a_cv_call_s"]), 3)
                    row["d_over_18a"] = round(min(ts) / (18 * min(row["a_cv_call_s"])), 4)
            print(json.dumps(row), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
