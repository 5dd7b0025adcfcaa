#!/usr/bin/env python3
"""Generator of tests/golden/call_sharp_cells.json: the cells on which the variant caller's score is compared between depth 200 and the depth cap.

    python tools/call_sharp_cells.py [--out tests/golden/call_sharp_cells.json] [--jobs 8] [--check]

Runs on the CPU alone.  Three lists:
  sharp      per depth (200, 5,000, 5,001, 2^14, 2^16, 2^18, 2^20 - 1, 2^20) and background e = A / B near 1e-3, 1e-2, 0.3, 0.5 and 0.9: one candidate whose
             high-precision score (tests/call_ref.py::hp_phred) lies between 2e-6 and 2e-5 ABOVE an integer and one that lies as far BELOW one, so that a bias of
             either sign of more than 2e-6 in the device's score flips a floor.  k runs from one above expectation to mean + 8 sigma; every score is below the cap.
             The search draws (k, K_o, N_o, prior) at random, scores a batch with tests/call_host.cpp - the host functions of call_model.h, built here WITHOUT
             sanitizers, for speed - and confirms every hit of the host with hp_phred; a hit the reference does not confirm is dropped.
  loop_end   ordinary cells under e = 0.999 at n = 20,000 and 2^20 with k in {n - 17, n - 16, n - 15, n - 1, n}: the last round of 16 lanes runs into i > n.
  near_one   ordinary cells with e = (B - 1) / B, B = 10^6 and B = 2^31 - 1 + 2^30 (the largest pool sum under the largest prior), k = n; depths 5,000 and
             2^20, and 2^18 and 2^20 (at 5,000 the score under the larger B is 7e-6: not an ordinary cell).
Every cell carries its prior (a0, n0) and its score as a decimal string with 30 places.  Each (depth, background) pair has a random stream of its own, seeded by
(SEED, depth, index of the background), and takes the first hit of each sign in draw order: the file is the same byte for byte whatever --jobs is.  --check
regenerates and compares with the committed file instead of writing.

Measured: 4.0 million host evaluations (200 batches of 20,000; the hit rate is about 2e-5 per draw and sign) and 80 confirmations, none refused, in 18 s of wall
time with --jobs 8 and 40 s with --jobs 3: 2 CPU-minutes, of which the pairs at n >= 2^18 and e >= 0.3 take most (thousands of terms per tail)."""
import argparse
import decimal
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import call_ref as CR  # noqa: E402

SEED = 41400
CAP = CR.MAX_DEPTH
DEPTHS = [200, 5000, 5001, 1 << 14, 1 << 16, 1 << 18, CAP - 1, CAP]
BACKGROUNDS = [1e-3, 1e-2, 0.3, 0.5, 0.9]
PRIORS = [(1, 997), (3, 2999)]                     # no powers of ten: under 1 / 1000 alone every k = n cell scores an integer
BAND = (decimal.Decimal("2e-6"), decimal.Decimal("2e-5"))
HOST_BAND = (2.05e-6, 1.95e-5)                     # what the host's double must show before the reference is asked (its error is below 1e-8)
BATCH = 20000
FILTERS = dict(min_depth=1, min_alt=1, min_ppm=0, min_q=0, bg_max_ppm=10 ** 6)
text = CR.hp_text


def side(score: decimal.Decimal) -> int:
    """+1: the score lies within the band above an integer; -1: below one; 0: neither."""
    nearest = score.to_integral_value(rounding=decimal.ROUND_HALF_EVEN)
    d = score - nearest
    return (1 if d > 0 else -1) if BAND[0] <= abs(d) <= BAND[1] else 0


def build_host(folder: str) -> str:
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed"
    exe = os.path.join(folder, "call_host")
    subprocess.run([gxx, "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "call_host.cpp")], check=True)
    return exe


def host_scores(exe: str, folder: str, tag: str, cells):
    """The host's score of every (k, n, K_o, N_o, a0, n0), through one run of call_host."""
    path = os.path.join(folder, f"cases_{tag}.txt")
    with open(path, "w") as f:
        for k, n, K_o, N_o, a0, n0 in cells:
            f.write(f"5 {n - k} {k} 0 0 0 {K_o} {N_o} 1 0 1 1 0 0 {a0} {n0} 1000000\n")
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, check=True).stdout.split(b"\n")
    return [float(l.split()[4]) if l.split()[0] == b"1" else None for l in out[:len(cells)]]


def draw(rng, n: int, e: float):
    a0, n0 = PRIORS[int(rng.integers(0, len(PRIORS)))]
    N_o = int(rng.integers(0, 50_000)) if e < 5e-3 else int(rng.integers(10_000, 2_000_000))
    B = N_o + n0
    A = max(a0, min(B - 1, int(round(B * e * float(rng.uniform(0.97, 1.03))))))
    K_o = A - a0
    mean, sigma = n * A / B, math.sqrt(n * A / B * (1 - A / B))
    lo, hi = int(mean) + 1, min(n, max(int(mean) + 1, int(mean + 8 * sigma)))
    return int(rng.integers(lo, hi + 1)), n, K_o, N_o, a0, n0


def search(job):
    """One (depth, background) pair: the first draw of each sign that the reference confirms."""
    exe, folder, n, ei = job
    e = BACKGROUNDS[ei]
    rng = np.random.default_rng([SEED, n, ei])
    found, tries, confirmations = {}, 0, 0
    while len(found) < 2:
        cells = [draw(rng, n, e) for _ in range(BATCH)]
        for cell, h in zip(cells, host_scores(exe, folder, f"{n}_{ei}", cells)):
            tries += 1
            if h is None or h >= CR.Q_CAP - 1:
                continue
            d = h - round(h)
            s = 1 if d > 0 else -1
            if not HOST_BAND[0] <= abs(d) <= HOST_BAND[1] or s in found:
                continue
            k, n_, K_o, N_o, a0, n0 = cell
            assert CR.candidate(k, n_, K_o, N_o, dict(FILTERS, a0=a0, n0=n0))
            score = CR.hp_phred(k, n_, K_o + a0, N_o + n0)
            confirmations += 1
            if side(score) == s:
                found[s] = dict(n=n_, k=k, K_o=K_o, N_o=N_o, a0=a0, n0=n0, e=e, side=s, hp=text(score))
    return [found[1], found[-1]], tries, confirmations


def ordinary(n: int, k: int, K_o: int, N_o: int, a0: int, n0: int) -> dict:
    assert CR.candidate(k, n, K_o, N_o, dict(FILTERS, a0=a0, n0=n0))
    score = CR.hp_phred(k, n, K_o + a0, N_o + n0)
    assert score < CR.Q_CAP and abs(score - score.to_integral_value()) > decimal.Decimal("1e-4")      # ordinary: far from every floor
    return dict(n=n, k=k, K_o=K_o, N_o=N_o, a0=a0, n0=n0, hp=text(score))


def generate(jobs: int):
    with tempfile.TemporaryDirectory() as folder:
        exe = build_host(folder)
        todo = [(exe, folder, n, ei) for n in DEPTHS for ei in range(len(BACKGROUNDS))]
        with ProcessPoolExecutor(jobs) as pool:
            results = list(pool.map(search, sorted(todo, key=lambda j: -j[2] * BACKGROUNDS[j[3]])))   # (the slow pairs first; the order of the file is DEPTHS x BACKGROUNDS)
        by_job = {(j[2], j[3]): r for j, r in zip(sorted(todo, key=lambda j: -j[2] * BACKGROUNDS[j[3]]), results)}
    sharp, tries, confirmations = [], 0, 0
    for n in DEPTHS:
        for ei in range(len(BACKGROUNDS)):
            cells, t, c = by_job[(n, ei)]
            sharp += cells
            tries += t
            confirmations += c
    # e = 999,000 / 1,000,000 under the prior 1 / 997
    loop_end = [ordinary(n, n - back, 998_999, 999_003, 1, 997) for n in (20_000, CAP) for back in (17, 16, 15, 1, 0)]
    top = (1 << 31) - 1
    near_one = [ordinary(n, n, 999_003, 999_003, 996, 997) for n in (5000, CAP)] + [ordinary(n, n, top, top, (1 << 30) - 1, 1 << 30) for n in (1 << 18, CAP)]
    head = dict(seed=SEED, filters=FILTERS, band=[str(BAND[0]), str(BAND[1])])
    lists = [f' "{name}": [\n' + ",\n".join("  " + json.dumps(c) for c in cells) + "\n ]" for name, cells in (("sharp", sharp), ("loop_end", loop_end), ("near_one", near_one))]
    body = "{\n" + ",\n".join([f' "{key}": {json.dumps(value)}' for key, value in head.items()] + lists) + "\n}\n"       # (a cell per line)
    return body, tries, confirmations


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "call_sharp_cells.json"))
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--check", action="store_true", help="regenerate and compare with --out instead of writing it")
    args = ap.parse_args()
    t0 = time.time()
    body, tries, confirmations = generate(args.jobs)
    print(f"{tries} host evaluations, {confirmations} confirmations, {time.time() - t0:.0f} s", file=sys.stderr)
    if args.check:
        same = open(args.out).read() == body
        print("identical" if same else "DIFFERENT", file=sys.stderr)
        return 0 if same else 1
    with open(args.out, "w") as f:
        f.write(body)
    return 0


if __name__ == "__main__":
    sys.exit(main())
