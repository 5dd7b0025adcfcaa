#!/usr/bin/env python3
"""Cost of the tag merge (mipgen_accel_reads_set_tag_mismatches) on the family1 and family8 legs of tools/consensus_rate.py (2 x 100 bases, tags 5,0,
85 % captured molecules, a quality string per read), with 1 % of the pairs given one substituted tag base, at tag mismatches 0 and 1 of the same build.  The
pairs are fed in calls of 10^6 (four distinct chunks per leg, cycled, with fresh tags in every call; making them is not timed).  After a warm-up session every
(leg, d) runs `--repeats` times.  One JSON line per leg, d and repetition: HIP-event time of k_tag_parent + k_tag_root + k_tag_rewrite
(mipgen_accel_last_kernel_ms 18), of both sorts and run boundaries (10), of the two vote kernels (9), the wall time of finish, and the merge totals; a last line
per (leg, d) gives the medians and the spread (max - min) / median over the repetitions.  Measured; no gate.

    python tools/tag_merge_rate.py [--pairs 10000000] [--probes 100000] [--repeats 3]
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
from consensus_rate import BASES, make_chunk, set_tags  # noqa: E402
from read_count_rate import CHUNK, READ_LEN, TE, make_probes  # noqa: E402

LEGS = ("family1", "family8")
TAG_ERROR_RATE = 0.01


def substitute_tags(ext, rng):
    """One tag base of 1 % of the pairs replaced by another of A C G T."""
    hit = np.flatnonzero(rng.random(len(ext)) < TAG_ERROR_RATE)
    at = rng.integers(0, TE, len(hit))
    code = np.searchsorted(BASES, ext[hit, at])
    ext[hit, at] = BASES[(code + rng.integers(1, 4, len(hit))) & 3]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000000)
    ap.add_argument("--probes", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    genome = synth.random_genome(4000000, 11)
    acc = capi.Accel(capi.make_params(152, 162, score_method=capi.SCORE_LOGISTIC), device=0)
    acc.set_timing(True)
    lib, h = acc.lib, acc.h
    i64p = C.POINTER(C.c_int64)
    n_probes = a.probes
    arms, start, stop = make_probes(genome, n_probes, rng)
    arr = (capi.Probe * n_probes)()
    for i, q in enumerate(arms):
        arr[i] = capi.Probe(q[0], q[1], None, None, 0, 0, -1, 0)
    off = np.arange(CHUNK + 1, dtype=np.int64) * READ_LEN
    pool = BASES[rng.integers(0, 4, (11, TE))]
    for leg in LEGS:
        chunks = []
        for _ in range(4):
            p = rng.integers(0, n_probes, CHUNK)
            chunks.append((p,) + make_chunk(genome, start, stop, p, rng))
        for d in (0, 1):
            runs = []
            for rep in range(-1, a.repeats):                                       # -1: the warm-up session
                tag_rng = np.random.default_rng(1000 + rep)                        # the same tags at d = 0 and d = 1
                acc._check(lib.mipgen_accel_reads_open_consensus(h, arr, n_probes, TE, 0, 0, None, 0, 0, 0))
                if d:
                    acc.set_tag_mismatches(d)
                fed = 0
                while fed < a.pairs:
                    c = min(CHUNK, a.pairs - fed)
                    p, e, l, eq, lq = chunks[(fed // CHUNK) % len(chunks)]
                    set_tags(e, p, leg, None, pool, tag_rng)
                    substitute_tags(e, tag_rng)
                    acc._check(lib.mipgen_accel_reads_feed_consensus(h, c, e.ctypes.data, eq.ctypes.data, off.ctypes.data_as(i64p), l.ctypes.data, lq.ctypes.data,
                                                                     off.ctypes.data_as(i64p), None, None))
                    fed += c
                unique = np.empty(n_probes, dtype=np.int64)
                tot, sizes = capi.ReadTotals(), capi.ConsensusSizes()
                t2 = time.perf_counter()
                acc._check(lib.mipgen_accel_reads_finish_consensus(h, None, unique.ctypes.data_as(i64p), C.byref(tot), None, None, C.byref(sizes)))
                finish_ms = (time.perf_counter() - t2) * 1e3
                if rep < 0:
                    continue
                merge = acc.last_tag_merge()
                assert int(unique.sum()) == sizes.n_groups == merge["groups"] and merge["raw_groups"] - merge["groups"] == merge["absorbed"]
                run = {"leg": leg, "d": d, "rep": rep, "probes": n_probes, "pairs": a.pairs, "members": int(tot.assigned - tot.tag_n), **merge,
                       "tag_merge_ms": round(acc.last_kernel_ms(18), 4), "sort_ms": round(acc.last_kernel_ms(10), 4), "k_consensus_vote_ms": round(acc.last_kernel_ms(9), 4),
                       "finish_ms": round(finish_ms, 2)}
                runs.append(run)
                print(json.dumps(run), flush=True)
            summary = {"leg": leg, "d": d, "summary": True}
            for key in ("tag_merge_ms", "sort_ms", "k_consensus_vote_ms", "finish_ms"):
                v = np.array([r[key] for r in runs])
                med = float(np.median(v))
                summary[key + "_median"] = round(med, 4)
                summary[key + "_spread"] = round(float(v.max() - v.min()) / med, 4) if med > 0 else None
            print(json.dumps(summary), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
