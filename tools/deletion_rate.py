#!/usr/bin/env python3
"""Rate of the deletion alleles (mipgen_accel_reads_consensus_deletions) on the legs of tools/gapped_pileup_rate.py - family1, family8, skewed -
with a deletion of 1 to 5 bases planted in the extension reads of 0 %, 2 % and 20 % of the molecules (chosen by a hash of probe and tag, so that the members
of a family agree).  Per leg and share: the session fed and
finished as there, one gapped pileup (max_indel 8) and then `--calls` deletions calls of the one row on the same consensus reads.  One JSON line per leg, share,
repetition and call: the HIP-event time of the deletions call's kernels (mipgen_accel_last_kernel_ms 19) beside that of the gapped pileup of the same session
(index 12), the events and the alleles of the call.  Measured; no gate.

    python tools/deletion_rate.py [--pairs 10000000] [--probes 100000] [--repeats 1] [--calls 3] [--shares 0,0.02,0.2]
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
from read_count_rate import CHUNK, READ_LEN, TE, make_probes  # noqa: E402


def plant_deletions(e0, p, share, rng):
    """A copy of the extension reads e0 (tags set) that lack 1..5 bases in the rows a hash of (probe, tag) picks; random bases fill the read's end."""
    e = e0.copy()
    if share <= 0:
        return e
    tag = np.zeros(len(p), dtype=np.uint64)
    for j in range(TE):
        tag = tag * np.uint64(5) + e0[:, j].astype(np.uint64)
    key = (p.astype(np.uint64) * np.uint64(1315423911) + tag) * np.uint64(2654435761) % np.uint64(1 << 32)
    chosen = key < np.uint64(int(share * (1 << 32)))
    for k in range(1, 6):
        sel = np.flatnonzero(chosen & (key % np.uint64(5) == np.uint64(k - 1)))
        if len(sel) == 0:
            continue
        c = TE + 35 + 7 * k                                                     # behind tag and arm, in front of the read's end
        e[sel, c:READ_LEN - k] = e0[sel, c + k:]
        e[sel, READ_LEN - k:] = BASES[rng.integers(0, 4, (len(sel), k))]
    return e


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000000)
    ap.add_argument("--probes", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--shares", default="0,0.02,0.2")
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
    mol_seq = b"".join(genome[s:t] for s, t in zip(start.tolist(), stop.tolist())).upper()
    n_pos = int(mol_len.sum())
    counts = np.empty((n_pos, 8), dtype=np.int32)
    gapped = np.empty((n_pos, 8), dtype=np.int32)
    sites = np.empty((n_pos, 4), dtype=np.int32)
    arr = (capi.Probe * n_probes)()
    for i, q in enumerate(arms):
        arr[i] = capi.Probe(q[0], q[1], None, None, 0, 0, -1, 0)
    off = np.arange(CHUNK + 1, dtype=np.int64) * READ_LEN
    pool = BASES[rng.integers(0, 4, (11, TE))]
    giant = np.zeros(n_probes, dtype=bool)
    giant[rng.choice(n_probes, min(N_GIANT, n_probes), replace=False)] = True
    giant_ids = np.flatnonzero(giant)
    for leg in a.legs.split(","):
        chunks = []
        for _ in range(4):
            p = rng.integers(0, n_probes, CHUNK)
            if leg == "skewed":
                hot = rng.random(CHUNK) < 0.01 / 0.85
                p[hot] = giant_ids[rng.integers(0, len(giant_ids), int(hot.sum()))]
            chunks.append((p,) + make_chunk(genome, start, stop, p, rng))
        for share in [float(x) for x in a.shares.split(",")]:
            for rep in range(-1 if share == 0 else 0, a.repeats):                  # -1: the warm-up session
                acc._check(lib.mipgen_accel_reads_open_consensus(h, arr, n_probes, TE, 0, 0, None, 0, 0, 0))
                fed = 0
                while fed < a.pairs:
                    c = min(CHUNK, a.pairs - fed)
                    p, e, l, eq, lq = chunks[(fed // CHUNK) % len(chunks)]
                    set_tags(e, p, leg, giant, pool, rng)
                    ev = plant_deletions(e, p, share, rng)
                    acc._check(lib.mipgen_accel_reads_feed_consensus(h, c, ev.ctypes.data, eq.ctypes.data, off.ctypes.data_as(i64p), l.ctypes.data, lq.ctypes.data,
                                                                     off.ctypes.data_as(i64p), None, None))
                    fed += c
                sizes = capi.ConsensusSizes()
                acc._check(lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, C.byref(sizes)))
                gt = capi.GappedTotals()
                acc._check(lib.mipgen_accel_reads_consensus_pileup_gapped(h, mol_seq, mol_len.ctypes.data_as(i32p), n_probes, 0, 1, 0, 8, gapped.ctypes.data_as(i32p),
                                                                          C.byref(gt)))
                gapped_ms = acc.last_kernel_ms(12)
                for call in range(a.calls if rep >= 0 else 1):
                    tot = capi.DeletionTotals()
                    t0 = time.perf_counter()
                    acc._check(lib.mipgen_accel_reads_consensus_deletions(h, mol_seq, mol_len.ctypes.data_as(i32p), n_probes, 0, 1, 0, 8, counts.ctypes.data_as(i32p),
                                                                          sites.ctypes.data_as(i32p), C.byref(tot)))
                    wall_s = time.perf_counter() - t0
                    ms = acc.last_kernel_ms(19)
                    if rep < 0:
                        continue
                    assert tot.groups == tot.used == sizes.n_groups and tot.deleted_bases == gt.deletions == int(sites[:, 3].sum(dtype=np.int64))
                    assert tot.events == int(sites[:, 1].sum(dtype=np.int64)) and counts.tobytes() == gapped.tobytes()
                    assert acc.last_kernel_ms(12) == gapped_ms
                    records = acc.deletions_fetch(int(tot.alleles))
                    assert int(records["count"].sum(dtype=np.int64)) == tot.events
                    print(json.dumps({
                        "leg": leg, "share": share, "probes": n_probes, "pairs": a.pairs, "rep": rep, "call": call, "groups": int(sizes.n_groups), "positions": n_pos,
                        "deletions_ms": round(ms, 4), "gapped_ms": round(gapped_ms, 4), "events": int(tot.events), "alleles": int(tot.alleles),
                        "ragged": int(tot.ragged), "deleted_bases": int(tot.deleted_bases), "depth": int(tot.depth), "gapped_sides": int(tot.gapped_sides),
                        "call_wall_ms": round(wall_s * 1e3, 2)}), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
