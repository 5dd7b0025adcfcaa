#!/usr/bin/env python3
"""Rate of the per-sample read counter (mipgen_accel_reads_open_samples / _feed_samples / _finish_samples) on the synthetic pairs of
tools/read_count_rate.py (2 x 100 bases, tags 5,0, 85 % captured molecules) with an index read per pair: 8 bases over 96 samples and 8 + 8 bases over
1,536 samples, barcodes drawn pairwise >= 3 apart, samples at uneven depth, 3 % of the indices with one substitution; barcode_mismatches 0 and 1.  The
pairs are fed in calls of 10^6 (four distinct chunks, cycled; making them is not timed).  After a warm-up session every leg runs `--repeats` times.  One
JSON line per leg and repetition: HIP-event time of k_sample_assign and of k_read_assign (with rows) summed over the feed calls
(mipgen_accel_last_kernel_ms 8 and 7), wall time of open, of the feed calls and of finish.  Measured; no gate.

    python tools/sample_count_rate.py [--pairs 10000000] [--probes 10000] [--repeats 2]
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
from read_count_rate import CHUNK, READ_LEN, TE, make_chunk, make_probes  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
LEGS = [(96, 8), (1536, 16)]           # samples, index bases (16 = 8 + 8)


def draw_barcodes(rng, n, J):
    kept = np.zeros((0, J), dtype=np.uint8)
    while len(kept) < n:
        c = rng.integers(0, 4, J).astype(np.uint8)
        if len(kept) == 0 or int((kept != c[None, :]).sum(axis=1).min()) >= 3:
            kept = np.vstack([kept, c[None, :]])
    return kept                                                           # codes 0..3


def make_indices(codes, n, rng):
    """[n][J] index bytes: the barcode of a sample drawn at uneven depth, 3 % with one substitution."""
    w = rng.random(len(codes)) ** 2 + 0.01
    idx = codes[rng.choice(len(codes), n, p=w / w.sum())]
    sub = np.flatnonzero(rng.random(n) < 0.03)
    pos = rng.integers(0, codes.shape[1], len(sub))
    idx[sub, pos] = (idx[sub, pos] + rng.integers(1, 4, len(sub))) & 3
    return np.ascontiguousarray(BASES[idx])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="10000000")
    ap.add_argument("--probes", default="10000")
    ap.add_argument("--repeats", type=int, default=2)
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
        for n_samples, J in LEGS:
            codes = draw_barcodes(rng, n_samples, J)
            assert len({c.tobytes() for c in codes}) == n_samples
            barcodes = [BASES[c].tobytes() for c in codes]
            bc = (C.c_char_p * n_samples)(*barcodes)
            indices = [make_indices(codes, CHUNK, rng) for _ in range(4)]
            ioff = np.arange(CHUNK + 1, dtype=np.int64) * J
            cells = (n_samples + 1) * n_probes
            for d in (0, 1):
                for n_pairs in [int(s) for s in a.pairs.split(",")]:
                    for rep in range(-1, a.repeats):                       # -1: the warm-up session
                        t0 = time.perf_counter()
                        acc._check(lib.mipgen_accel_reads_open_samples(h, arr, n_probes, TE, 0, 0, bc, n_samples, d))
                        t1 = time.perf_counter()
                        fed = 0
                        while fed < n_pairs:
                            c = min(CHUNK, n_pairs - fed)
                            k = (fed // CHUNK) % len(chunks)
                            e, l = chunks[k]
                            acc._check(lib.mipgen_accel_reads_feed_samples(h, c, e.ctypes.data, off.ctypes.data_as(i64p), l.ctypes.data, off.ctypes.data_as(i64p),
                                                                           indices[k].ctypes.data, ioff.ctypes.data_as(i64p)))
                            fed += c
                        t2 = time.perf_counter()
                        sample_ms, assign_ms = acc.last_kernel_ms(8), acc.last_kernel_ms(7)
                        reads = np.empty(cells, dtype=np.int64)
                        unique = np.empty(cells, dtype=np.int64)
                        row_pairs = np.empty(n_samples + 1, dtype=np.int64)
                        tot, stot = capi.ReadTotals(), capi.SampleTotals()
                        acc._check(lib.mipgen_accel_reads_finish_samples(h, reads.ctypes.data_as(i64p), unique.ctypes.data_as(i64p), C.byref(tot), C.byref(stot),
                                                                         row_pairs.ctypes.data_as(i64p)))
                        t3 = time.perf_counter()
                        if rep < 0:
                            continue
                        assert int(reads.sum()) == tot.assigned and int(row_pairs.sum()) == tot.pairs == n_pairs
                        print(json.dumps({
                            "probes": n_probes, "samples": n_samples, "index_bases": J, "barcode_mismatches": d, "pairs": n_pairs, "rep": rep, "assigned": int(tot.assigned),
                            "sample_none": int(stot.sample_none), "sample_ambiguous": int(stot.sample_ambiguous), "unique_tags": int(unique.sum()),
                            "k_sample_assign_ms": round(sample_ms, 4), "k_read_assign_ms": round(assign_ms, 4), "open_ms": round((t1 - t0) * 1e3, 2),
                            "feed_wall_ms": round((t2 - t1) * 1e3, 2), "finish_ms": round((t3 - t2) * 1e3, 2),
                            "pairs_per_s_sample_kernel": round(n_pairs / (sample_ms * 1e-3), 0) if sample_ms > 0 else None,
                            "pairs_per_s_wall": round(n_pairs / (t3 - t1), 0)}), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
