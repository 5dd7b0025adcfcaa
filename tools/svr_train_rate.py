#!/usr/bin/env python3
"""Training rate of the device SVR trainer (mipgen_accel_train_svr) against the reference's libsvm (svm_train + svm_save_model on one CPU core,
oracle ref_svm_train_save), on feature rows of real candidates (tests/test_gpu_svr_train.py's training_set).  Prints one JSON line per size:
the kernel-matrix build (HIP events) and the solver (wall time), the iteration count, us per iteration, the Gram kernel's share of the FP64
vector peak, the libsvm time, and whether the two model files are identical.

    python tools/svr_train_rate.py [--sizes 2000,8000,20000] [--gamma G] [--cost C] [--p P] [--no-ref]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mipgen_amd import capi, synth  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests.test_gpu_svr_train import ref_model, training_set  # noqa: E402

FP64_VECTOR_PEAK_TFLOPS = 78.6     # MI355X: 256 CUs x 128 FP64 vector flop/clk (FMA = 2) x 2.4 GHz


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,8000,20000")
    ap.add_argument("--gamma", type=float, default=1 / 192)
    ap.add_argument("--cost", type=float, default=8.0)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=101)
    ap.add_argument("--no-ref", action="store_true", help="skip the libsvm run")
    a = ap.parse_args()
    P = capi.make_params(130, 140, score_method=capi.SCORE_SVR, arm_pairs=synth.arm_pairs_from_sums([43, 44, 45]))
    acc = capi.Accel(P, device=0)
    with tempfile.TemporaryDirectory() as tmp:
        Xw, Yw = training_set(300, a.seed)                                  # warm-up: the first launches load the code objects
        acc.train_svr(Xw, Yw, a.gamma, a.cost, a.p, model_path=os.path.join(tmp, "warm.model"))
        for n in (int(s) for s in a.sizes.split(",")):
            X, Y = training_set(n, a.seed + n)
            ours = os.path.join(tmp, f"ours_{n}.model")
            t0 = time.perf_counter()
            info = acc.train_svr(X, Y, a.gamma, a.cost, a.p, model_path=ours)
            wall = time.perf_counter() - t0
            tiles = (n + 15) // 16
            dot_flops = tiles * (tiles + 1) / 2 * 256 * 192 * 2            # the upper-triangle tiles' dot products (exp not counted)
            row = {"n": n, "gamma": a.gamma, "C": a.cost, "p": a.p, "gram_ms": round(info["gram_ms"], 3), "solve_ms": round(info["solve_ms"], 1),
                   "iterations": info["iterations"], "us_per_iter": round(1e3 * info["solve_ms"] / max(info["iterations"], 1), 2),
                   "n_sv": info["n_sv"], "n_shrink": info["n_shrink"], "n_reconstruct": info["n_reconstruct"], "device_wall_s": round(wall, 3),
                   "gram_dot_share_of_fp64_peak": round(dot_flops / (info["gram_ms"] * 1e-3) / (FP64_VECTOR_PEAK_TFLOPS * 1e12), 4)}
            if not a.no_ref and po.have_refdrv():
                t0 = time.perf_counter()
                want = ref_model(X, Y, a.gamma, a.cost, a.p, os.path.join(tmp, f"ref_{n}.model"))
                row["libsvm_s"] = round(time.perf_counter() - t0, 3)
                row["identical"] = open(ours, "rb").read() == want
                row["speedup"] = round(row["libsvm_s"] / wall, 1)
            print(json.dumps(row), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
