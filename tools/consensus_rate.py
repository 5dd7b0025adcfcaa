#!/usr/bin/env python3
"""Rate of the consensus reads (mipgen_accel_reads_open_consensus / _feed_consensus / _finish_consensus) on the synthetic pairs of
tools/read_count_rate.py (2 x 100 bases, tags 5,0, 85 % captured molecules) with a quality string per read, in three legs:
  family1   a random tag per pair: nearly every molecule is read once;
  family8   eleven tags per probe: 10^5 probes x 10^7 pairs give a mean family of about 8;
  skewed    family1 with 1 % of the pairs in 100 giant families (100 probes, one tag each): the workgroup kernel.
The pairs are fed in calls of 10^6 (four distinct chunks per leg, cycled, with fresh tags in every call; making them is not timed).  After a warm-up session
every leg runs `--repeats` times.  One JSON line per leg and repetition: HIP-event time of the two k_consensus_vote kernels (mipgen_accel_last_kernel_ms 9), the
bytes they move - both reads and both quality strings of every member behind the tag, its 32-byte record and pair id, two bytes per consensus position - as a
share of the achievable HBM rate, the sort and run boundaries (mipgen_accel_last_kernel_ms 10), k_read_assign summed over the feed calls, and the wall time of
the feed calls and of finish.  Measured; no gate.

    python tools/consensus_rate.py [--pairs 10000000] [--probes 100000] [--repeats 2]
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
from read_count_rate import _COMP, CHUNK, HBM_ACHIEVABLE, READ_LEN, TE, make_probes  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
LEGS = ("family1", "family8", "skewed")
N_GIANT = 100


def make_chunk(genome, start, stop, p, rng):
    """The pairs of read_count_rate.make_chunk for the probes `p`: tag + M[:95] and revcomp(M)[:100], 15 % random extension reads; and two quality matrices."""
    g = np.frombuffer(genome, dtype=np.uint8)
    n = len(p)
    cols = np.arange(READ_LEN)
    ext = g[start[p][:, None] + cols[None, :READ_LEN - TE]]
    lig = _COMP[g[stop[p][:, None] - 1 - cols[None, :]]]
    ext = np.concatenate([BASES[rng.integers(0, 4, (n, TE))], ext], axis=1)
    noise = rng.random(n) < 0.15
    ext[noise] = BASES[rng.integers(0, 4, (int(noise.sum()), READ_LEN))]
    qual = [rng.integers(35, 75, (n, READ_LEN)).astype(np.uint8) for _ in range(2)]
    return np.ascontiguousarray(ext), np.ascontiguousarray(lig), qual[0], qual[1]


def set_tags(ext, p, leg, giant, pool, rng):
    """Fresh tags for one feed call, by the leg's rule."""
    n = len(p)
    if leg == "family8":
        ext[:, :TE] = pool[rng.integers(0, len(pool), n)]
    else:
        ext[:, :TE] = BASES[rng.integers(0, 4, (n, TE))]
        if leg == "skewed":
            ext[giant[p], :TE] = ord("A")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000000)
    ap.add_argument("--probes", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=2)
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
    giant = np.zeros(n_probes, dtype=bool)
    giant[rng.choice(n_probes, min(N_GIANT, n_probes), replace=False)] = True
    giant_ids = np.flatnonzero(giant)
    for leg in LEGS:
        chunks = []
        for _ in range(4):
            p = rng.integers(0, n_probes, CHUNK)
            if leg == "skewed":
                hot = rng.random(CHUNK) < 0.01 / 0.85                              # (15 % of the extension reads are random bases)
                p[hot] = giant_ids[rng.integers(0, len(giant_ids), int(hot.sum()))]
            chunks.append((p,) + make_chunk(genome, start, stop, p, rng))
        for rep in range(-1, a.repeats):                                           # -1: the warm-up session
            t0 = time.perf_counter()
            acc._check(lib.mipgen_accel_reads_open_consensus(h, arr, n_probes, TE, 0, 0, None, 0, 0, 0))
            open_s = time.perf_counter() - t0
            fed, feed_s = 0, 0.0
            while fed < a.pairs:
                c = min(CHUNK, a.pairs - fed)
                p, e, l, eq, lq = chunks[(fed // CHUNK) % len(chunks)]
                set_tags(e, p, leg, giant, pool, rng)
                t1 = time.perf_counter()
                acc._check(lib.mipgen_accel_reads_feed_consensus(h, c, e.ctypes.data, eq.ctypes.data, off.ctypes.data_as(i64p), l.ctypes.data, lq.ctypes.data,
                                                                 off.ctypes.data_as(i64p), None, None))
                feed_s += time.perf_counter() - t1
                fed += c
            assign_ms = acc.last_kernel_ms(7)
            reads = np.empty(n_probes, dtype=np.int64)
            unique = np.empty(n_probes, dtype=np.int64)
            tot, sizes = capi.ReadTotals(), capi.ConsensusSizes()
            t2 = time.perf_counter()
            acc._check(lib.mipgen_accel_reads_finish_consensus(h, reads.ctypes.data_as(i64p), unique.ctypes.data_as(i64p), C.byref(tot), None, None, C.byref(sizes)))
            finish_s = time.perf_counter() - t2
            vote_ms, sort_ms = acc.last_kernel_ms(9), acc.last_kernel_ms(10)
            if rep < 0:
                continue
            family = np.empty(sizes.n_groups, dtype=np.int32)
            acc._check(lib.mipgen_accel_reads_consensus_fetch(h, None, None, family.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None, None, None))
            members = int(tot.assigned - tot.tag_n)
            assert int(unique.sum()) == sizes.n_groups and int(family.sum()) == members
            moved = members * (2 * (2 * READ_LEN - TE) + 36) + 2 * (sizes.ext_bytes + sizes.lig_bytes)
            print(json.dumps({
                "leg": leg, "probes": n_probes, "pairs": a.pairs, "rep": rep, "members": members, "groups": int(sizes.n_groups), "mean_family": round(members / max(sizes.n_groups, 1), 3),
                "largest_family": int(family.max()) if len(family) else 0, "workgroup_families": int((family > 256).sum()),
                "k_consensus_vote_ms": round(vote_ms, 4), "vote_bytes": moved, "vote_share_of_hbm": round(moved / (vote_ms * 1e-3) / HBM_ACHIEVABLE, 4) if vote_ms > 0 else None,
                "sort_ms": round(sort_ms, 4), "k_read_assign_ms": round(assign_ms, 4), "open_ms": round(open_s * 1e3, 2), "feed_wall_ms": round(feed_s * 1e3, 2),
                "finish_ms": round(finish_s * 1e3, 2), "pairs_per_s_feed_and_finish": round(a.pairs / (feed_s + finish_s), 0)}), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
