#!/usr/bin/env python3
"""Rate of the locus calls (mipgen_accel_reads_consensus_locus_plan / _locus_pileup / _locus_call_pool / _locus_call) on the three legs of
tools/call_rate.py - family1, family8, skewed, 96 sample rows, a variant planted in 1 % of the (sample, probe) cells - with every probe overlapping its neighbour
by half: probe k covers 160 bases from 1000 + 80 k, arms of 20, so every target base but those at the two ends is covered by two probes (or by one probe's target
and the next one's arm, which the plan leaves out).  Per leg: the plan, then three pileups of row 0, one pool, then `--calls` calls of each of `--rows` rows.  One
JSON line per leg and repetition: HIP-event time of index 14 for plan, pileup, pool and call - median and spread (max - min) of three - the candidates and calls
per call.  Measured; no gate.

    python tools/locus_rate.py [--pairs 10000000] [--probes 10000] [--repeats 1] [--calls 3] [--rows 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mipgen_amd import capi, synth  # noqa: E402
from consensus_rate import BASES, LEGS, N_GIANT, make_chunk, set_tags  # noqa: E402
from read_count_rate import CHUNK, READ_LEN, TE  # noqa: E402
from sample_count_rate import draw_barcodes  # noqa: E402

N_SAMPLES, J, PLANT_AT, PLANT_SHARE = 96, 8, 40, 0.01
FIRST, STEP, ARM, LENGTH = 1000, 80, 20, 160


def tiled_probes(genome, n):
    """n probes of LENGTH bases, each STEP behind the one before; the plan of their targets and the ref bytes of the loci."""
    g = np.frombuffer(genome, dtype=np.uint8)
    start = FIRST + STEP * np.arange(n, dtype=np.int64)
    arms = [(g[s:s + ARM].tobytes(), g[s + LENGTH - ARM:s + LENGTH].tobytes()) for s in start.tolist()]
    t = np.arange(LENGTH, dtype=np.int64)
    locus = start[:, None] + t[None, :] - (FIRST + ARM)
    plan = np.where((t >= ARM) & (t < LENGTH - ARM), locus * 4, -1).astype(np.int64).reshape(-1)
    n_loci = int(locus[-1, LENGTH - ARM - 1]) + 1
    return arms, start, start + LENGTH, np.ascontiguousarray(plan), genome[FIRST + ARM:FIRST + ARM + n_loci].upper()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000000)
    ap.add_argument("--probes", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rows", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    genome = synth.random_genome(4000000, 11)
    acc = capi.Accel(capi.make_params(152, 162, score_method=capi.SCORE_LOGISTIC), device=0)
    acc.set_timing(True)
    lib, h = acc.lib, acc.h
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    n_probes = a.probes
    arms, start, stop, plan, locus_ref = tiled_probes(genome, n_probes)
    mol_len = np.ascontiguousarray(stop - start, dtype=np.int32)
    g = np.frombuffer(genome, dtype=np.uint8)
    arr = (capi.Probe * n_probes)()
    for i, q in enumerate(arms):
        arr[i] = capi.Probe(q[0], q[1], None, None, 0, 0, -1, 0)
    codes = draw_barcodes(rng, N_SAMPLES, J)
    barcodes = [BASES[c].tobytes() for c in codes]
    bc = (C.c_char_p * N_SAMPLES)(*barcodes)
    planted = rng.random((N_SAMPLES, n_probes)) < PLANT_SHARE                          # the (sample, probe) cells that carry the variant
    off = np.arange(CHUNK + 1, dtype=np.int64) * READ_LEN
    idx_off = np.arange(CHUNK + 1, dtype=np.int64) * J
    pool = BASES[rng.integers(0, 4, (11, TE))]
    giant = np.zeros(n_probes, dtype=bool)
    giant[rng.choice(n_probes, min(N_GIANT, n_probes), replace=False)] = True
    giant_ids = np.flatnonzero(giant)
    prm = capi.CallParams(min_depth=4, min_alt=2)                                      # (10^7 pairs over 96 x 10,000 cells: some 9 molecules per cell)
    for leg in LEGS:
        chunks = []
        for _ in range(4):
            p = rng.integers(0, n_probes, CHUNK)
            if leg == "skewed":
                hot = rng.random(CHUNK) < 0.01 / 0.85
                p[hot] = giant_ids[rng.integers(0, len(giant_ids), int(hot.sum()))]
            s = rng.integers(0, N_SAMPLES, CHUNK)
            e, l, eq, lq = make_chunk(genome, start, stop, p, rng)
            hit = planted[s, p]
            e[hit, TE + PLANT_AT] = BASES[(np.searchsorted(BASES, g[start[p[hit]] + PLANT_AT]) + 1) & 3]
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
            ref = np.frombuffer(locus_ref, dtype=np.uint8)
            plan_ms, pile_ms, pool_ms, ms, cands, calls = [], [], [], [], [], []
            for _ in range(3):
                acc._check(lib.mipgen_accel_reads_consensus_locus_plan(h, plan.ctypes.data_as(i64p), len(plan), ref.ctypes.data, len(ref)))
                plan_ms.append(acc.last_kernel_ms(14))
            for _ in range(3):
                acc._check(lib.mipgen_accel_reads_consensus_locus_pileup(h, None, mol_len.ctypes.data_as(i32p), n_probes, 0, 1, 0, 0, None, None, None, None))
                pile_ms.append(acc.last_kernel_ms(14))
            for _ in range(3 if rep >= 0 else 1):
                acc._check(lib.mipgen_accel_reads_consensus_locus_call_pool(h, None, mol_len.ctypes.data_as(i32p), n_probes, 1, 0, 0, prm.bg_max_ppm))
                pool_ms.append(acc.last_kernel_ms(14))
            for row in range(min(a.rows, N_SAMPLES) if rep >= 0 else 1):
                for _ in range(a.calls if rep >= 0 else 1):
                    tot = capi.CallTotals()
                    acc._check(lib.mipgen_accel_reads_consensus_locus_call(h, row, C.byref(prm), None, None, C.byref(tot)))
                    ms.append(acc.last_kernel_ms(14)); cands.append(int(tot.candidates)); calls.append(int(tot.calls))
            if rep < 0:
                continue
            med, spread = (lambda v: round(statistics.median(v), 4)), (lambda v: round(max(v) - min(v), 4))
            print(json.dumps({
                "leg": leg, "probes": n_probes, "pairs": a.pairs, "samples": N_SAMPLES, "rep": rep, "groups": int(sizes.n_groups), "positions": int(mol_len.sum()),
                "loci": len(ref), "planted_cells": int(planted.sum()), "plan_ms_median": med(plan_ms), "plan_ms_spread": spread(plan_ms), "pileup_ms_median": med(pile_ms),
                "pileup_ms_spread": spread(pile_ms), "pool_ms_median": med(pool_ms), "pool_ms_spread": spread(pool_ms), "call_ms_median": med(ms), "call_ms_spread": spread(ms),
                "candidates_per_call": round(statistics.mean(cands), 1), "calls_per_call": round(statistics.mean(calls), 1)}), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
