#!/usr/bin/env python3
"""Rate of the sequence route against the coordinate route on the SAME candidates: the condensed survivors of the synthetic 1,000 x 5 kb workload
(workloads.regions5k), scored by mipgen_accel_score_probes from their sequences and by mipgen_accel_score_candidates from their coordinates.  After
a warm-up call of each, every leg runs twice, alternating.  Prints one JSON line per list size and leg: HIP-event time of the feature kernel and of
k_svr_gemm (mipgen_accel_last_kernel_ms 6 / 5), whole-call wall time, candidates per second of both, and whether the two routes' scores are the same
bits.  The sequence route's wall time includes packing and uploading every base of every probe; the coordinate route reads a resident batch.

    python tools/probe_rate.py [--sizes 10000,100000,1000000] [--sv 1024]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mipgen_amd import capi, synth, workloads  # noqa: E402

_RC = bytes.maketrans(b"ACGT", b"TGCA")


def survivors_as_candidates(P, grids, surv, limit):
    """Condensed survivors (batch-wide dense indices) -> (region, scan_start, capture_size, ext_len, lig_len, strand), the first `limit` of them."""
    pairs = capi.arm_pairs_of(P)
    A = len(pairs)
    idx = surv["cand_index"][surv["cand_index"] >= 0][:limit]
    offs = np.array([g.offset for g in grids], dtype=np.int64)
    reg = np.searchsorted(offs, idx, side="right") - 1
    out = []
    for i, r in zip(idx.tolist(), reg.tolist()):
        g = grids[r]
        local = i - g.offset
        row, a = divmod(local, A)
        rest, strand = divmod(row, 2)
        pi, ki = divmod(rest, g.n_sizes)
        e, l = pairs[a]
        out.append((r, g.first_pos + pi, P.max_capture_size - (g.first_size_index + ki) * P.capture_increment, e, l, strand))
    return out


def as_probes(regions, cands, copies):
    out = []
    for (r, p, Cs, e, l, strand), (ec, lc) in zip(cands, copies):
        rd = regions[r]; ss = Cs - e - l; o = rd.c.seq_start
        es, ls = (p - e, p + ss) if strand == 0 else (p + ss, p - l)
        ext, lig, ins = rd.seq[es - o:es - o + e], rd.seq[ls - o:ls - o + l], rd.seq[p - o:p - o + ss]
        if strand:
            ext, lig, ins = ext.translate(_RC)[::-1], lig.translate(_RC)[::-1], ins.translate(_RC)[::-1]
        out.append((ext, lig, ins, None, ec, lc, r))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--sv", type=int, default=1024)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    n_regions = max(2, -(-max(sizes) // 9000))                             # ~10^4 survivors per 5 kb region
    P = capi.make_params(152, 162, score_method=capi.SCORE_SVR)
    acc = capi.Accel(P, device=0)
    with tempfile.TemporaryDirectory() as tmp:
        genome, ivs = workloads.regions5k(n_regions)
        acc.load_model_file(workloads.svr_model_path(tmp, genome, a.sv))
        regions = workloads.build_regions5k(acc, genome, ivs, P)
        grids = acc.upload(regions)
        acc.score_condense_all(capi.SCORE_LOGISTIC)
        _, surv = acc.download_survivors()
        cands_all = survivors_as_candidates(P, grids, surv, max(sizes))
        acc.set_timing(True)
        lrc = np.array([[rd.c.long_range_content[k] for k in range(capi.N_LRC)] for rd in regions])
        for n in sizes:
            cands = cands_all[:n]
            if len(cands) < n:
                print(json.dumps({"n": n, "error": f"only {len(cands)} survivors"}), flush=True)
                continue
            arr = (capi.Candidate * n)(*[capi.Candidate(*c) for c in cands])
            ints = acc.score_candidates(cands[:min(n, 200000)], capi.SCORE_LOGISTIC, want_ints=True)[3] if n <= 200000 else None
            copies = [(ints[i].ext_copy, ints[i].lig_copy) for i in range(n)] if ints is not None else \
                [(x.ext_copy, x.lig_copy) for c0 in range(0, n, 200000) for x in acc.score_candidates(cands[c0:c0 + 200000], capi.SCORE_LOGISTIC, want_ints=True)[3]]
            probes = as_probes(regions, cands, copies)
            parr = (capi.Probe * n)(*[capi.Probe(q[0], q[1], q[2], q[3], q[4], q[5], q[6], 0) for q in probes])
            dp = capi.C.POINTER(capi.C.c_double)
            s_c, s_p = np.empty(n), np.empty(n)
            bases = sum(len(q[0]) + len(q[1]) + len(q[2]) for q in probes)

            def leg_coord():
                t0 = time.perf_counter()
                acc._check(acc.lib.mipgen_accel_score_candidates(acc.h, arr, n, capi.SCORE_SVR, s_c.ctypes.data_as(dp), None, None, None))
                return time.perf_counter() - t0

            def leg_probe():
                t0 = time.perf_counter()
                acc._check(acc.lib.mipgen_accel_score_probes(acc.h, parr, n, lrc.ctypes.data_as(dp), lrc.shape[0], capi.SCORE_SVR, s_p.ctypes.data_as(dp), None, None))
                return time.perf_counter() - t0

            leg_coord(); leg_probe()                                           # warm-up: code objects, buffers
            for rep in range(2):
                for name, leg in (("score_candidates", leg_coord), ("score_probes", leg_probe)):
                    wall = leg()
                    feat_ms, svr_ms = acc.last_kernel_ms(6), acc.last_kernel_ms(5)
                    print(json.dumps({"n": n, "leg": name, "rep": rep, "feature_kernel_ms": round(feat_ms, 4), "svr_gemm_ms": round(svr_ms, 4),
                                      "wall_ms": round(1e3 * wall, 3), "feature_kernel_cands_per_s": round(n / (feat_ms * 1e-3)),
                                      "wall_cands_per_s": round(n / wall), "probe_bases": bases,
                                      "feature_kernel_GBps_read_plus_written": round((bases * (name == "score_probes") + n * 192 * 8) / (feat_ms * 1e-3) / 1e9, 1)}),
                          flush=True)
            print(json.dumps({"n": n, "scores_bit_identical": bool(np.array_equal(s_c.view(np.int64), s_p.view(np.int64))),
                              "max_abs_diff": float(np.max(np.abs(s_c - s_p)))}), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
