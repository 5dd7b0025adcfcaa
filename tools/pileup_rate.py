#!/usr/bin/env python3
"""Rate of the pileup (mipgen_accel_reads_consensus_pileup) on the consensus reads of the three legs of tools/consensus_rate.py - family1, family8,
skewed: the same synthetic pairs (2 x 100 bases, tags 5,0, 85 % captured molecules, molecules of 132 to 191 bases), fed and finished as there; then a pileup of
every row (without barcodes: one) at min_family 1, min_quality 0, `--calls` times on the same consensus reads.  After a warm-up session every leg runs
`--repeats` times.  One JSON line per leg, repetition and call: HIP-event time of the pileup kernels (mipgen_accel_last_kernel_ms 11: cell boundaries,
partition, the two count kernels, the column sums), the bytes the model says they move - the consensus bases and qualities of both sides once, 36 bytes of
offsets and family per group, 20 bytes written per template position - as a share of the achievable HBM rate, and the wall time of the call with its download
of the table.  Measured; no gate.

    python tools/pileup_rate.py [--pairs 10000000] [--probes 100000] [--repeats 2] [--calls 2]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mipgen_amd import capi, synth  # noqa: E402
from consensus_rate import BASES, LEGS, N_GIANT, make_chunk, set_tags  # noqa: E402
from read_count_rate import CHUNK, HBM_ACHIEVABLE, READ_LEN, TE, make_probes  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000000)
    ap.add_argument("--probes", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--calls", type=int, default=2)
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
    n_pos = int(mol_len.sum())
    counts = np.empty((n_pos, 5), dtype=np.int32)
    arr = (capi.Probe * n_probes)()
    for i, q in enumerate(arms):
        arr[i] = capi.Probe(q[0], q[1], None, None, 0, 0, -1, 0)
    off = np.arange(CHUNK + 1, dtype=np.int64) * READ_LEN
    pool = BASES[rng.integers(0, 4, (11, TE))]
    giant = np.zeros(n_probes, dtype=bool)
    giant[rng.choice(n_probes, min(N_GIANT, n_probes), replace=False)] = True
    giant_ids = np.flatnonzero(giant)
    for leg in LEGS:
        chunks = []
        for _ in range(4):
            p = rng.integers(0, n_probes, CHUNK)
            if leg == "skewed":
                hot = rng.random(CHUNK) < 0.01 / 0.85
                p[hot] = giant_ids[rng.integers(0, len(giant_ids), int(hot.sum()))]
            chunks.append((p,) + make_chunk(genome, start, stop, p, rng))
        for rep in range(-1, a.repeats):                                           # -1: the warm-up session
            acc._check(lib.mipgen_accel_reads_open_consensus(h, arr, n_probes, TE, 0, 0, None, 0, 0, 0))
            fed = 0
            while fed < a.pairs:
                c = min(CHUNK, a.pairs - fed)
                p, e, l, eq, lq = chunks[(fed // CHUNK) % len(chunks)]
                set_tags(e, p, leg, giant, pool, rng)
                acc._check(lib.mipgen_accel_reads_feed_consensus(h, c, e.ctypes.data, eq.ctypes.data, off.ctypes.data_as(i64p), l.ctypes.data, lq.ctypes.data,
                                                                 off.ctypes.data_as(i64p), None, None))
                fed += c
            unique = np.empty(n_probes, dtype=np.int64)
            sizes = capi.ConsensusSizes()
            acc._check(lib.mipgen_accel_reads_finish_consensus(h, None, unique.ctypes.data_as(i64p), None, None, None, C.byref(sizes)))
            vote_ms = acc.last_kernel_ms(9)
            for call in range(a.calls if rep >= 0 else 1):
                tot = capi.PileupTotals()
                t0 = time.perf_counter()
                acc._check(lib.mipgen_accel_reads_consensus_pileup(h, mol_len.ctypes.data_as(i32p), n_probes, 0, 1, 0, counts.ctypes.data_as(i32p), C.byref(tot)))
                wall_s = time.perf_counter() - t0
                ms = acc.last_kernel_ms(11)
                if rep < 0:
                    continue
                assert tot.groups == tot.used == sizes.n_groups and tot.bases == int(counts[:, :4].sum(dtype=np.int64)) and tot.discordant == int(counts[:, 4].sum(dtype=np.int64))
                moved = 2 * (sizes.ext_bytes + sizes.lig_bytes) + 36 * sizes.n_groups + 20 * n_pos
                print(json.dumps({
                    "leg": leg, "probes": n_probes, "pairs": a.pairs, "rep": rep, "call": call, "groups": int(sizes.n_groups), "positions": n_pos,
                    "largest_cell": int(unique.max()), "workgroup_cells": int((unique > 256).sum()), "bases": int(tot.bases), "discordant": int(tot.discordant),
                    "pileup_ms": round(ms, 4), "pileup_bytes": moved, "pileup_share_of_hbm": round(moved / (ms * 1e-3) / HBM_ACHIEVABLE, 4) if ms > 0 else None,
                    "groups_per_s": round(sizes.n_groups / (ms * 1e-3), 0) if ms > 0 else None, "call_wall_ms": round(wall_s * 1e3, 2),
                    "k_consensus_vote_ms": round(vote_ms, 4)}), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
