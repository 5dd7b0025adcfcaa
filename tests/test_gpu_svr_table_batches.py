"""GPU: k_svr_dense's factor-table batches, bit for bit, where the batch numbering of the table stage can go wrong.  The table stage hands out batches of
64 entries from one counter whose index space is  [0, nU_pad) upstream windows | [nU_pad, nU_pad + nD_pad) downstream windows | inserts  (pads to 64,
common.h: svr_table_ranges): an entry that is decoded twice, skipped, or decoded with the other role's constants moves a factor and with it the score of
every candidate that uses it.  Scores (as int64 words) and records are compared through SHA-256 with tests/golden/svr_table_batches.json, which was recorded
from the build BEFORE the numbering was changed (`python tests/test_gpu_svr_table_batches.py --record` on a GPU rewrites it - only ever from a build whose
scores are the accepted ones).

The shapes, by accel_tiles.hip's rules (256 lanes per pair chunk, capture increment 5, the default pairs: 12 upstream and 12 downstream arm lengths):

  stub5 / stub6 / stub16   capture 140-180 -> kc = 9 capture sizes, np = 256 / 9 = 28, lowered to 27 (27 + 5 = 0 mod 32), ssr = 46.  A region of 707, 708, 718
           positions is 27 tiles: 26 of np = 27 (nU = 324 = five batches and four entries, nD = 864) and a last tile of np = 5, 6, 16:
           nU = 60 (less than one batch), 72 (one batch and a piece of eight), 192 (exactly three batches: no idle lane before the downstream range);
           nD = 600, 612, 732; inserts 230, 276, 736 (lane -> (position, scan size) wraps every 46 lanes)
  kc2      capture 150-155 -> kc = 2, ssr = 11: the insert decode wraps five or six times inside a batch (64 = 5 x 11 + 9), at other lanes in every batch;
           320 positions = 5 tiles of np = 64 (LDS-bound np, evened out over the tiles): nU = 768, exactly twelve batches, nD = 888, inserts 704 = eleven batches
  kc4      capture 150-165 -> kc = 4, ssr = 21: three or four wraps per batch; 330 positions = 6 tiles of np = 55: nU = 660, nD = 900, inserts 1,155
           (the walk of tests/svr_table_decode.cpp covers every np at these capture ranges: the two cases do not hinge on the exact tile shape)
  uneven   the pairs (16,24) (17,24) (18,24) (16,25): 3 extension and 2 ligation lengths, so n_up != n_dn and the two strands swap them; capture 140-180

with 4 and 7 support vectors (one and two zero-padded partial groups).  Both strands are part of every grid."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "svr_table_batches.json")
SAMPLE = 8                                   # words of the strided sample kept per array

pytestmark = pytest.mark.gpu

UNEVEN = [(18, 24), (16, 25), (17, 24), (16, 24)]          # enumeration order: sum descending, extension arm ascending
#        name          capture     pairs   regions (bed start, bed end)   n_sv
CASES = [("stub5_sv4", (140, 180), None, [(5000, 5573)], 4),
         ("stub6_sv7", (140, 180), None, [(5000, 5574)], 7),
         ("stub16_sv4", (140, 180), None, [(5000, 5584)], 4),
         ("kc2_sv7", (150, 155), None, [(3000, 3211)], 7),
         ("kc4_sv4", (150, 165), None, [(3000, 3211)], 4),
         ("uneven_sv7", (140, 180), UNEVEN, [(3000, 3166)], 7)]
EXPECT_POSITIONS = {"stub5_sv4": [707], "stub6_sv7": [708], "stub16_sv4": [718]}


def _genome():
    from mipgen_amd import synth
    return synth.random_genome(12000, 11, n_run_frac=0.002, n_run_len=6)


def _run_case(case, tmpdir):
    """-> (positions per region, scores as int64 words, records) of one case, scored through the C ABI"""
    from mipgen_amd import capi, synth
    name, (cmin, cmax), pairs, beds, n_sv = case
    genome = _genome()
    P = capi.make_params(cmin, cmax, score_method=capi.SCORE_SVR, max_mip_overlap=30, arm_pairs=pairs)
    model = os.path.join(tmpdir, f"svr_table_batches_{n_sv}.model")
    if not os.path.exists(model):
        synth.synthetic_svr_model(model, genome, n_sv, seed=5)
    regions = [capi.build_region(genome, "1", b0, b1, P, bwa_mode="hashed", label=f"r{i}", lrc=np.linspace(0.01 + 0.1 * i, 0.3, 44))
               for i, (b0, b1) in enumerate(beds)]
    acc = capi.Accel(P, device=0)
    try:
        acc.load_model_file(model)
        acc.set_sv_split(1)
        grids, scores, records = acc.score_regions(regions, capi.SCORE_SVR)
    finally:
        acc.close()
    assert sum(g.count for g in grids) == scores.size == records.size
    return [int(g.n_pos) for g in grids], np.ascontiguousarray(scores).view(np.int64), np.ascontiguousarray(records).view(np.uint64)


def _summary(n_pos, words, records):
    def one(a):
        idx = np.linspace(0, a.size - 1, SAMPLE).astype(np.int64)
        return {"n": int(a.size), "sha256": hashlib.sha256(a.tobytes()).hexdigest(), "at": [int(i) for i in idx], "words": [f"{int(w) & (2 ** 64 - 1):016x}" for w in a[idx]]}
    return {"positions": n_pos, "scores": one(words), "records": one(records), "nan_scores": int(np.isnan(words.view(np.float64)).sum())}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_table_batches_keep_every_bit(case, golden, tmp_path_factory):
    tmpdir = str(tmp_path_factory.getbasetemp())
    n_pos, words, records = _run_case(case, tmpdir)
    got, want = _summary(n_pos, words, records), golden[case[0]]
    if case[0] in EXPECT_POSITIONS:                                   # the grids are the ones whose tile shapes the docstring lists
        assert n_pos == EXPECT_POSITIONS[case[0]]
    assert got["positions"] == want["positions"]
    assert got["nan_scores"] == want["nan_scores"]
    assert want["scores"]["n"] > 2 * want["nan_scores"], "the recording scores mostly real candidates"
    for what in ("records", "scores"):
        g, w = got[what], want[what]
        assert g["n"] == w["n"]
        if g["sha256"] != w["sha256"]:
            diff = [(i, a, b) for i, a, b in zip(w["at"], g["words"], w["words"]) if a != b]
            pytest.fail(f"{case[0]}: {what} differ from the recording (sha256 {g['sha256'][:16]} != {w['sha256'][:16]}); sampled words that differ "
                        f"(index, got, recorded): {diff[:4] or 'none of the sample'}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_svr_table_batches.py --record   (rewrites tests/golden/svr_table_batches.json from this build, on a GPU)")
    import tempfile
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for c in CASES:
            out[c[0]] = _summary(*_run_case(c, td))
            print(c[0], out[c[0]]["positions"], out[c[0]]["scores"]["n"], out[c[0]]["scores"]["sha256"][:16], "NaN", out[c[0]]["nan_scores"], flush=True)
    with open(os.environ.get("SVR_TABLE_BATCHES_OUT", GOLDEN), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
