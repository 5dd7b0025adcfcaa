"""GPU: the bounds skips of mipgen.cpp:443-444 where they cut - at the first and the last bases of a chromosome - through every kernel that decides or
reads them (mip_bounds.h: the literal rule in k_records_logistic, the row form in k_logistic_dense, the span form in k_replay_condense_narrow; the record's
VALID bit in k_replay_condense and k_replay_condense_carry).  Two regions of the 20,000-base golden genome in ONE upload, BED (10, 270) and (19740, 19995):
at the start the lower clause leaves scan positions with no or only some constructed candidates, at the end the upper clause cuts (position, size, pair)
triples by the hundred thousand, and the second region has a non-zero offset into the result arrays.  Each parameter set reaches one code path (SETS);
all run in one child process, the oracle's dense scores of every (set, region) computed beside it on a few threads.

Per set, against oracle/pyoracle.py: grid geometry equal, records bit-equal, scores within 1e-5 (NaN and inf in the same places), emitted count and mask
equal replay_region's, the survivors' cand_index / record / score equal condense_region's (both fed the device's own scores, as everywhere in the suite)."""
import concurrent.futures
import faulthandler
import json
import os
import subprocess
import sys
import time
import traceback

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
BEDS = (("start", 10, 270), ("end", 19740, 19995))
# name: (min capture, max capture, increment, arm pairs (None: the default 57, else a key of test_gpu_fuzz._pair_lists), method); all with the heuristic on
SETS = {
    "K1_carry3": (150, 150, 5, None, "logistic"),
    "K3_carry3": (150, 160, 5, None, "logistic"),
    "K4_carry5": (150, 165, 5, None, "logistic"),
    "K5_carry5": (150, 170, 5, None, "logistic"),
    "K8_carry8": (150, 185, 5, None, "logistic"),
    "K9_narrow": (150, 190, 5, None, "logistic"),
    "K16_narrow": (150, 225, 5, None, "logistic"),
    "K17_narrow_wide": (150, 230, 5, None, "logistic"),
    "K4_A65_chunked": (150, 165, 5, "A65", "logistic"),
    "K17_A65_chunked": (150, 230, 5, "A65", "logistic"),
    "K4_step50_records_logistic_scores": (120, 270, 50, None, "logistic"),      # the window tables of k_logistic_dense do not fit: k_records_logistic<true>
    "K5_svr_records_logistic_no_scores": (150, 170, 5, None, "svr"),            # k_records_logistic<false> feeds k_svr_dense
}


def _inputs(name):
    from mipgen_amd import capi
    from tests import helpers as H
    from tests.test_gpu_fuzz import _pair_lists
    lo, hi, inc, pairs, method = SETS[name]
    m = capi.SCORE_SVR if method == "svr" else capi.SCORE_LOGISTIC
    P = capi.make_params(lo, hi, score_method=m, capture_increment=inc, arm_pairs=_pair_lists()[pairs] if pairs else None)
    genome = H.golden_genome()
    assert len(genome) == 20000
    regions = [capi.build_region(genome, "1", b0, b1, P, bwa_mode="hashed", label=label) for label, b0, b1 in BEDS]
    return P, m, regions


def check_set(name, P, method, regions, refs, model_path):
    from mipgen_amd import capi
    from oracle import pyoracle as po
    acc = capi.Accel(P)
    try:
        if method == capi.SCORE_SVR:
            acc.load_model_file(model_path)
        grids, scores, records = acc.score_regions(regions, method)
        acc.replay_condense()
        emitted, surv, mask = acc.download_replay()
    finally:
        acc.close()
    assert grids[0].offset == 0 and grids[1].offset == grids[0].count > 0
    pos0, figures = 0, {}
    for ri, (rd, g) in enumerate(zip(regions, grids)):
        og, os_, or_ = refs[ri].result()
        label = BEDS[ri][0]
        # the condition on the inputs, from the oracle's records alone: the bounds skips cut some candidates of the region, not all
        o_valid = (capi.rec_flags(or_) & capi.FLAG_VALID) != 0
        assert 0 < int(o_valid.sum()) < og.count, (name, label)
        per_pos = o_valid.reshape(og.n_pos, -1).sum(axis=1)
        figures[label] = dict(candidates=int(og.count), constructed=int(o_valid.sum()), positions_none=int((per_pos == 0).sum()),
                              positions_partly=int(((per_pos > 0) & (per_pos < og.count // og.n_pos)).sum()))
        assert (g.first_pos, g.n_pos, g.first_size_index, g.n_sizes, g.count) == (og.first_pos, og.n_pos, og.first_size_index, og.n_sizes, og.count), (name, label)
        r, s = records[g.offset:g.offset + g.count], np.asarray(scores[g.offset:g.offset + g.count])
        bad = np.flatnonzero(r != or_)
        assert bad.size == 0, (name, label, "records", int(bad.size), int(bad[0]), hex(int(r[bad[0]])), hex(int(or_[bad[0]])))
        assert np.array_equal(np.isnan(s), np.isnan(os_)) and np.array_equal(np.isinf(s), np.isinf(os_)), (name, label, "NaN / inf positions")
        inf = np.isinf(os_)
        assert np.array_equal(s[inf], os_[inf]), (name, label, "sign of inf")
        fin = np.isfinite(os_)
        d = np.abs(s[fin] - os_[fin])
        assert d.size == 0 or float(d.max()) <= TOL, (name, label, "scores", float(d.max()))
        n_emit, omask = po.replay_region(P, rd, s, r)
        assert int(emitted[ri]) == n_emit, (name, label, "emitted", int(emitted[ri]), n_emit)
        assert np.array_equal(mask[g.offset:g.offset + g.count], omask), (name, label, "mask")
        osurv = po.condense_region(P, rd, s, r, omask)
        got = surv[2 * pos0:2 * (pos0 + g.n_pos)]
        assert np.array_equal(got["cand_index"], np.where(osurv["cand_index"] >= 0, osurv["cand_index"] + g.offset, -1)), (name, label, "cand_index")
        assert np.array_equal(got["record"], osurv["record"]), (name, label, "survivor records")
        assert np.array_equal(got["score"], osurv["score"], equal_nan=True), (name, label, "survivor scores")
        pos0 += g.n_pos
    if name == "K17_narrow_wide":
        assert figures["start"]["positions_none"] == 20 and figures["start"]["positions_partly"] == 9, figures
    return figures


# ---- the child: every set on one device context; the first trouble on the device ends the run -------------------------------------------------------
def worker(out_path):
    from mipgen_amd import capi
    from oracle import pyoracle as po
    from tests import helpers as H
    faulthandler.dump_traceback_later(240, exit=True)
    results = {}
    model_path = os.path.join(H.GOLDEN, "models", "svr_syn_64.model")
    om = po.Model(model_path)
    inputs = {name: _inputs(name) for name in SETS}
    trouble = None
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        # the slowest references first (SVR, then by grid size)
        order = sorted(SETS, key=lambda n: (SETS[n][4] != "svr", -(SETS[n][1] - SETS[n][0]) // SETS[n][2]))
        refs = {}
        for name in order:
            P, m, regions = inputs[name]
            refs[name] = [pool.submit(po.score_region_dense, P, rd, m, om if m == capi.SCORE_SVR else None) for rd in regions]
        for name in SETS:
            if trouble:
                results[name] = dict(ok=False, error="not run: " + trouble)
                continue
            t0 = time.time()
            try:
                P, m, regions = inputs[name]
                results[name] = dict(ok=True, figures=check_set(name, P, m, regions, refs[name], model_path))
            except capi.AccelError as e:
                trouble = f"{name} met trouble on the device: {e}"
                results[name] = dict(ok=False, error=trouble)
            except Exception:
                results[name] = dict(ok=False, error=traceback.format_exc()[-3000:])
            results[name]["seconds"] = round(time.time() - t0, 3)
            print(name, results[name]["ok"], results[name]["seconds"], flush=True)
            with open(out_path + ".tmp", "w") as fh:
                json.dump(results, fh)
            os.replace(out_path + ".tmp", out_path)
            if trouble:
                for f in (f for fs in refs.values() for f in fs):
                    f.cancel()
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bounds_edges") / "verdicts.json")
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_bounds_edges", out], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    res = json.load(open(out)) if os.path.exists(out) else {}
    return res, f"the child ended with status {p.returncode}: {p.stdout.decode()[-3000:]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETS))
def test_parameter_set_at_the_chromosome_ends(verdicts, name):
    res, tail = verdicts
    assert name in res, f"{name} was not reached; {tail}"
    assert res[name]["ok"], res[name]["error"]


@pytest.mark.gpu
def test_the_upper_clause_cuts_the_end_region_as_counted(verdicts):
    """57 pairs at 17 sizes: 160,021 of the end region's 425,391 (position, size, pair) triples are cut - counted from the oracle's records, both strands alike"""
    res, tail = verdicts
    assert res.get("K17_narrow_wide", {}).get("ok"), tail
    f = res["K17_narrow_wide"]["figures"]["end"]
    assert f["candidates"] == 2 * 425391 and f["candidates"] - f["constructed"] == 2 * 160021, f


if __name__ == "__main__":
    worker(sys.argv[1])
