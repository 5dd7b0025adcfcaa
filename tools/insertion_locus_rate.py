#!/usr/bin/env python3
"""Rate of the fold of insertion alleles to genome loci (mipgen_accel_reads_consensus_locus_insertions) on the legs of tools/insertion_rate.py -
family1, family8, skewed, an insertion of 1 to 5 bases planted in the extension reads of a share of the molecules - with every probe doubled by a minus-strand
twin: the twin of the probe on genome[s:t) is the probe on the same bases of the reverse strand, so its template is the reverse complement, and the plan gives
the two one locus per base (the twin's position t' is the locus of the plus probe's position len - 1 - t', with bit 0 and, from t' = 1 on, bit 1).  Per leg and
share: the session fed and finished as there over the doubled probe set, then `--calls` plain insertions calls and `--calls` locus insertions calls of the one row
on the same consensus reads.  One JSON line per leg and share: the HIP-event time of the locus insertions call's kernels (mipgen_accel_last_kernel_ms 17, the
insertions route of the row included) beside that of the plain insertions call of the same session (index 15), each as the median of the calls with its lowest
and highest value, and the records in (the row's alleles) and out (the locus alleles) per call.  Measured; no gate.

    python tools/insertion_locus_rate.py [--pairs 10000000] [--probes 100000] [--calls 3] [--shares 0,0.02,0.2] [--legs family1,family8,skewed]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mipgen_amd import capi, synth  # noqa: E402
from consensus_rate import BASES, LEGS, N_GIANT, make_chunk, set_tags  # noqa: E402
from insertion_rate import plant_insertions  # noqa: E402
from read_count_rate import CHUNK, READ_LEN, TE, make_probes  # noqa: E402

_COMP = np.zeros(256, dtype=np.uint8)
_COMP[list(b"ACGTN")] = list(b"TGCAN")


def doubled(genome, n, rng):
    """(both strands of the genome end to end, arms, start, stop of 2 n probes on it - probe n + i the minus-strand twin of probe i -, the plan, the loci)."""
    g = np.frombuffer(genome, dtype=np.uint8)
    both = np.concatenate([g, _COMP[g[::-1]]]).tobytes()
    arms, start, stop = make_probes(genome, n, rng)
    N = len(g)
    t_start, t_stop = 2 * N - stop, 2 * N - start
    t_arms = [(both[s:s + len(l)], both[t - len(e):t]) for (e, l), s, t in zip(arms, t_start.tolist(), t_stop.tolist())]
    lens = (stop - start).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    n_loci = int(off[-1])
    plus = np.arange(n_loci, dtype=np.int64) * 4
    t = np.arange(n_loci, dtype=np.int64) - np.repeat(off[:-1], lens)                     # the twin's own position t' inside its template
    minus = (np.repeat(off[:-1] + lens - 1, lens) - t) * 4 + 1 + 2 * (t >= 1)
    return both, arms + t_arms, np.concatenate([start, t_start]), np.concatenate([stop, t_stop]), np.concatenate([plus, minus]), n_loci


def spread(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000000)
    ap.add_argument("--probes", type=int, default=100000)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--shares", default="0,0.02,0.2")
    ap.add_argument("--legs", default=",".join(LEGS))
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    genome = synth.random_genome(4000000, 11)
    both, arms, start, stop, plan, n_loci = doubled(genome, a.probes, rng)
    n_probes = 2 * a.probes
    acc = capi.Accel(capi.make_params(152, 162, score_method=capi.SCORE_LOGISTIC), device=0)
    acc.set_timing(True)
    lib, h = acc.lib, acc.h
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    mol_len = np.ascontiguousarray(stop - start, dtype=np.int32)
    mol_seq = b"".join(both[s:t] for s, t in zip(start.tolist(), stop.tolist())).upper()
    n_pos = int(mol_len.sum())
    assert n_pos == len(plan) == 2 * n_loci
    locus_ref = np.frombuffer(mol_seq[:n_loci], dtype=np.uint8)                           # (the plus probes' own bases: no call reads them here)
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
            chunks.append((p,) + make_chunk(both, start, stop, p, rng))
        for k, share in enumerate(float(x) for x in a.shares.split(",")):
            acc._check(lib.mipgen_accel_reads_open_consensus(h, arr, n_probes, TE, 0, 0, None, 0, 0, 0))
            fed = 0
            while fed < a.pairs:
                c = min(CHUNK, a.pairs - fed)
                p, e, l, eq, lq = chunks[(fed // CHUNK) % len(chunks)]
                set_tags(e, p, leg, giant, pool, rng)
                ev = plant_insertions(e, p, share, rng)
                acc._check(lib.mipgen_accel_reads_feed_consensus(h, c, ev.ctypes.data, eq.ctypes.data, off.ctypes.data_as(i64p), l.ctypes.data, lq.ctypes.data,
                                                                 off.ctypes.data_as(i64p), None, None))
                fed += c
            sizes = capi.ConsensusSizes()
            acc._check(lib.mipgen_accel_reads_finish_consensus(h, None, None, None, None, None, C.byref(sizes)))
            acc._check(lib.mipgen_accel_reads_consensus_locus_plan(h, plan.ctypes.data_as(i64p), len(plan), locus_ref.ctypes.data, n_loci))
            plain_ms, locus_ms = [], []
            it, lt = capi.InsertionTotals(), capi.LocusInsertionTotals()
            args = (h, mol_seq, mol_len.ctypes.data_as(i32p), n_probes, 0, 1, 0, 8)
            for call in range(a.calls + (k == 0)):                                        # (the first call of each kind after a leg's first session is the warm-up)
                acc._check(lib.mipgen_accel_reads_consensus_insertions(*args, None, None, C.byref(it)))
                plain_ms.append(acc.last_kernel_ms(15))
            for call in range(a.calls + (k == 0)):
                acc._check(lib.mipgen_accel_reads_consensus_locus_insertions(*args, None, None, None, None, C.byref(lt)))
                locus_ms.append(acc.last_kernel_ms(17))
                assert acc.last_kernel_ms(15) == plain_ms[-1]
            assert lt.insertions <= it.insertions and lt.folded + lt.dropped >= it.alleles
            records = acc.locus_insertions_fetch(int(lt.alleles))
            assert int(records["count"].sum(dtype=np.int64)) == lt.insertions
            print(json.dumps({
                "leg": leg, "share": share, "probes": n_probes, "pairs": a.pairs, "calls": a.calls, "groups": int(sizes.n_groups), "positions": n_pos, "loci": n_loci,
                "insertions_ms_15": spread(plain_ms[-a.calls:]), "locus_insertions_ms_17": spread(locus_ms[-a.calls:]), "records_in": int(it.alleles),
                "records_out": int(lt.alleles), "folded": int(lt.folded), "dropped": int(lt.dropped), "events": int(it.insertions), "locus_events": int(lt.insertions)}),
                flush=True)
    acc.close()


if __name__ == "__main__":
    main()
