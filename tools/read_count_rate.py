#!/usr/bin/env python3
"""Rate of the read counter (mipgen_accel_reads_open / _feed / _finish) on synthetic pairs of 2 x 100 bases: probes cut from a random
genome (arms 16-30, targets 100-130), 85 % of the pairs captured molecules of a random probe (2 % of them with a substitution in an arm), the rest
random sequence; tags 5,0.  The pairs are fed in calls of 10^6 (four distinct chunks, cycled; making them is not timed).  After a warm-up session
every leg runs `--repeats` times.  One JSON line per leg: HIP-event time of k_read_assign summed over the feed calls (mipgen_accel_last_kernel_ms 7),
wall time of open, of the feed calls and of finish, pairs per second by kernel time and by wall time, and the bytes the kernel moves (read bytes +
offsets + assignment + keys written) as a fraction of the achievable HBM bandwidth (6.3 TB/s).

    python tools/read_count_rate.py [--pairs 1000000,10000000] [--probes 10000,100000] [--repeats 2] [--mismatches 0]
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

from mipgen_amd import capi, synth  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
READ_LEN, TE, CHUNK = 100, 5, 1000000
_COMP = np.zeros(256, dtype=np.uint8)
for a_, b_ in zip(b"ACGT", b"TGCA"):
    _COMP[a_] = b_


def make_probes(genome, n, rng):
    g = np.frombuffer(genome, dtype=np.uint8)
    start = rng.integers(0, len(g) - 400, n)
    e, l, t = rng.integers(16, 31, n), rng.integers(16, 31, n), rng.integers(100, 131, n)
    arms = [(g[s:s + a].tobytes(), g[s + a + c:s + a + c + b].tobytes()) for s, a, b, c in zip(start.tolist(), e.tolist(), l.tolist(), t.tolist())]
    return arms, start, start + e + t + l


def make_chunk(genome, start, stop, n, rng):
    """n pairs as two [n][100] byte matrices: tag + M[:95] and revcomp(M)[:100] of a random probe's molecule, or random bases."""
    g = np.frombuffer(genome, dtype=np.uint8)
    p = rng.integers(0, len(start), n)
    cols = np.arange(READ_LEN)
    ext = g[start[p][:, None] + cols[None, :READ_LEN - TE]]
    lig = _COMP[g[stop[p][:, None] - 1 - cols[None, :]]]
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    ext = np.concatenate([bases[rng.integers(0, 4, (n, TE))], ext], axis=1)
    noise = rng.random(n) < 0.15
    ext[noise] = bases[rng.integers(0, 4, (int(noise.sum()), READ_LEN))]
    sub = np.flatnonzero(rng.random(n) < 0.02)
    ext[sub, TE + rng.integers(0, 16, len(sub))] = ord("A")
    return np.ascontiguousarray(ext), np.ascontiguousarray(lig)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1000000,10000000")
    ap.add_argument("--probes", default="10000,100000")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--mismatches", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    genome = synth.random_genome(4000000, 11)
    acc = capi.Accel(capi.make_params(152, 162, score_method=capi.SCORE_LOGISTIC), device=0)
    acc.set_timing(True)
    lib, h = acc.lib, acc.h
    i64p = C.POINTER(C.c_int64)
    for n_probes in [int(s) for s in a.probes.split(",")]:
        arms, start, stop = make_probes(genome, n_probes, rng)
        arr = (capi.Probe * n_probes)()
        for i, q in enumerate(arms):
            arr[i] = capi.Probe(q[0], q[1], None, None, 0, 0, -1, 0)
        chunks = [make_chunk(genome, start, stop, CHUNK, rng) for _ in range(4)]
        off = np.arange(CHUNK + 1, dtype=np.int64) * READ_LEN
        for n_pairs in [int(s) for s in a.pairs.split(",")]:
            for rep in range(-1, a.repeats):                               # -1: the warm-up session
                t0 = time.perf_counter()
                acc._check(lib.mipgen_accel_reads_open(h, arr, n_probes, TE, 0, a.mismatches))
                t1 = time.perf_counter()
                fed = 0
                while fed < n_pairs:
                    c = min(CHUNK, n_pairs - fed)
                    e, l = chunks[(fed // CHUNK) % len(chunks)]
                    acc._check(lib.mipgen_accel_reads_feed(h, c, e.ctypes.data, off.ctypes.data_as(i64p), l.ctypes.data, off.ctypes.data_as(i64p)))
                    fed += c
                t2 = time.perf_counter()
                kernel_ms = acc.last_kernel_ms(7)
                reads = np.empty(n_probes, dtype=np.int64)
                unique = np.empty(n_probes, dtype=np.int64)
                tot = capi.ReadTotals()
                acc._check(lib.mipgen_accel_reads_finish(h, reads.ctypes.data_as(i64p), unique.ctypes.data_as(i64p), C.byref(tot)))
                t3 = time.perf_counter()
                if rep < 0:
                    continue
                moved = n_pairs * (2 * READ_LEN + 16 + 4) + int(tot.assigned - tot.tag_n) * 8
                print(json.dumps({
                    "probes": n_probes, "pairs": n_pairs, "rep": rep, "assigned": int(tot.assigned), "ambiguous": int(tot.ambiguous), "unassigned": int(tot.unassigned),
                    "overflow": int(tot.overflow), "unique_tags": int(unique.sum()), "k_read_assign_ms": round(kernel_ms, 4), "open_ms": round((t1 - t0) * 1e3, 2),
                    "feed_wall_ms": round((t2 - t1) * 1e3, 2), "finish_ms": round((t3 - t2) * 1e3, 2),
                    "pairs_per_s_kernel": round(n_pairs / (kernel_ms * 1e-3), 0) if kernel_ms > 0 else None,
                    "pairs_per_s_wall": round(n_pairs / (t3 - t1), 0), "bytes_moved": moved,
                    "fraction_of_achievable_hbm": round(moved / (kernel_ms * 1e-3) / HBM_ACHIEVABLE, 4) if kernel_ms > 0 else None}), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
