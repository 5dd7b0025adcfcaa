#!/usr/bin/env python3
"""Rate of the insertion calls (mipgen_accel_reads_consensus_insertion_pool / _insertion_call) on the three legs of tools/call_rate.py - family1,
family8, skewed - demultiplexed over 96 sample rows, with an insertion planted in 1 % of the (sample, probe) cells: every extension read of such a cell carries
two inserted bases behind template position 40.  Per leg: one pool (the insertions route of all 96 rows, appended, sorted and reduced on the device), then `--calls`
insertion calls of each of `--rows` rows.  One JSON line per leg and repetition: HIP-event time of index 16 for the pool and per call - median and spread (max - min)
of the calls -, the entries and alleles of the pool, the candidates and calls per call, and the wall time of a call.  Measured; no gate.

    python tools/insertion_call_rate.py [--pairs 10000000] [--probes 10000] [--repeats 1] [--calls 3] [--rows 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mipgen_amd import capi, synth  # noqa: E402
from consensus_rate import BASES, LEGS, N_GIANT, make_chunk, set_tags  # noqa: E402
from read_count_rate import CHUNK, READ_LEN, TE, make_probes  # noqa: E402
from sample_count_rate import draw_barcodes  # noqa: E402

N_SAMPLES, J, PLANT_AT, PLANT_LEN, PLANT_SHARE, W = 96, 8, 40, 2, 0.01, 8


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000000)
    ap.add_argument("--probes", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rows", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS))
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    genome = synth.random_genome(4000000, 11)
    acc = capi.Accel(capi.make_params(152, 162, score_method=capi.SCORE_LOGISTIC), device=0)
    acc.set_timing(True)
    lib, h = acc.lib, acc.h
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    n_probes = a.probes
    arms, start, stop = make_probes(genome, n_probes, rng)
    mol_len = np.ascontiguousarray(stop - start, dtype=np.int32)
    mol_seq = b"".join(genome[int(s):int(e)] for s, e in zip(start, stop)).upper()
    arr = (capi.Probe * n_probes)()
    for i, q in enumerate(arms):
        arr[i] = capi.Probe(q[0], q[1], None, None, 0, 0, -1, 0)
    codes = draw_barcodes(rng, N_SAMPLES, J)
    barcodes = [BASES[c].tobytes() for c in codes]
    bc = (C.c_char_p * N_SAMPLES)(*barcodes)
    planted = rng.random((N_SAMPLES, n_probes)) < PLANT_SHARE                          # the (sample, probe) cells that carry the insertion
    inserted = BASES[rng.integers(0, 4, (n_probes, PLANT_LEN))]                        # ... one allele per probe
    off = np.arange(CHUNK + 1, dtype=np.int64) * READ_LEN
    idx_off = np.arange(CHUNK + 1, dtype=np.int64) * J
    pool = BASES[rng.integers(0, 4, (11, TE))]
    giant = np.zeros(n_probes, dtype=bool)
    giant[rng.choice(n_probes, min(N_GIANT, n_probes), replace=False)] = True
    giant_ids = np.flatnonzero(giant)
    prm = capi.CallParams(min_depth=4, min_alt=2)                                      # (10^7 pairs over 96 x 10,000 cells: some 9 molecules per cell)
    for leg in a.legs.split(","):
        chunks = []
        for _ in range(4):
            p = rng.integers(0, n_probes, CHUNK)
            if leg == "skewed":
                hot = rng.random(CHUNK) < 0.01 / 0.85
                p[hot] = giant_ids[rng.integers(0, len(giant_ids), int(hot.sum()))]
            s = rng.integers(0, N_SAMPLES, CHUNK)
            e, l, eq, lq = make_chunk(genome, start, stop, p, rng)
            hit = np.flatnonzero(planted[s, p])
            c = TE + PLANT_AT
            e[hit, c + PLANT_LEN:] = e[hit, c:READ_LEN - PLANT_LEN]
            e[hit, c:c + PLANT_LEN] = inserted[p[hit]]
            chunks.append((p, e, l, eq, lq, np.ascontiguousarray(BASES[codes[s]])))
        for rep in range(-1, a.repeats):                                           # -1: the warm-up session
            acc._check(lib.mipgen_accel_reads_open_consensus(h, arr, n_probes, TE, 0, 0, bc, N_SAMPLES, 0, 0))
            fed = 0
            while fed < a.pairs:
                c = min(CHUNK, a.pairs - fed)
                p, e, l, eq, lq, idx = chunks[(fed // CHUNK) % len(chunks)]
                set_tags(e, p, leg, giant, pool, rng)
                acc._check(lib.mipgen_accel_reads_feed_consensus(h, c, e.ctypes.data, eq.ctypes.data, off.ctypes.data_as(i64p), l.ctypes.data, lq.ctypes.data,
                                                                 off.ctypes.data_as(i64p), idx.ctypes.data, idx_off.ctypes.data_as(i64p)))
                fed += c
            sizes = capi.ConsensusSizes()
            acc._check(lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, C.byref(sizes)))
            ptot = capi.InsertionPoolTotals()
            t0 = time.perf_counter()
            acc._check(lib.mipgen_accel_reads_consensus_insertion_pool(h, mol_seq, mol_len.ctypes.data_as(i32p), n_probes, 1, 0, W, prm.bg_max_ppm, C.byref(ptot)))
            pool_wall_s, pool_ms = time.perf_counter() - t0, acc.last_kernel_ms(16)
            ms, wall, cands, calls = [], [], [], []
            for row in range(min(a.rows, N_SAMPLES) if rep >= 0 else 1):
                for _ in range(a.calls if rep >= 0 else 1):
                    tot = capi.CallTotals()
                    t0 = time.perf_counter()
                    acc._check(lib.mipgen_accel_reads_consensus_insertion_call(h, row, C.byref(prm), None, None, None, C.byref(tot)))
                    wall.append(time.perf_counter() - t0); ms.append(acc.last_kernel_ms(16)); cands.append(int(tot.candidates)); calls.append(int(tot.calls))
            if rep < 0:
                continue
            print(json.dumps({
                "leg": leg, "probes": n_probes, "pairs": a.pairs, "samples": N_SAMPLES, "rep": rep, "groups": int(sizes.n_groups), "positions": int(mol_len.sum()),
                "planted_cells": int(planted.sum()), "pool_ms": round(pool_ms, 3), "pool_wall_ms": round(pool_wall_s * 1e3, 2), "entries": int(ptot.entries),
                "alleles": int(ptot.alleles), "call_ms_median": round(statistics.median(ms), 4), "call_ms_spread": round(max(ms) - min(ms), 4),
                "call_wall_ms_median": round(statistics.median(wall) * 1e3, 2), "candidates_per_call": round(statistics.mean(cands), 1),
                "calls_per_call": round(statistics.mean(calls), 1)}), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
