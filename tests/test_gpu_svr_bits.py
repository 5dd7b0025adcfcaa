"""GPU: the dense SVR kernel's scores and records, bit for bit, against a recording made before the candidate phase of k_svr_dense was re-laid
(position-minor insert table at a padded pitch; lanes without a candidate on rows of their own).  Such changes move data; the operands of
every multiply and FMA and their order are what they were, so every score must keep its last bit: scores.view(int64) and the records are compared
through SHA-256 digests (plus a strided sample of the words themselves, to say WHERE a difference starts).

tests/golden/svr_dense_bits.json is the recording (`python tests/test_gpu_svr_bits.py --record` on a GPU rewrites it - only ever from a build whose
scores are the accepted ones).  What the cases reach, by the tile shapes accel_tiles.hip lays out (lanes per pair chunk 256, capture increment 5):

  wide     capture 140-180 -> tiles of kc = 9 capture sizes: 300 positions = 12 tiles of np = 25 (lane pitch 27 != np, table pitch 33),
           703 positions = 26 tiles of np = 27 (lane pitch = np, table pitch 33) + one tile of np = 1 (table pitch 1); 57 pairs = k_svr_dense<15>,
           the last chunk holds 12 pairs; with 3, 4 and 7 support vectors (whole group, one and two zero-padded partial groups) and, for 7, cut in
           two along the SV list
  mid      capture 150-170 -> kc = 5: a region at the chromosome start (56 positions = 2 tiles of np = 28: the lanes do not allow a padded lane pitch
           and no odd table pitch spreads a lane pitch of 28 - the fallback np | 1 = 29; its first windows reach before the chromosome: bounds-skipped pairs)
           and 304 positions further in (np = 51)
  one      capture 150-150 -> kc = 1 (any odd pitch is conflict free): 304 positions = 4 tiles of np = 76
  pairs16  the first 16 pairs of the list (two arm sums) -> two chunks of 8, k_svr_dense<8>
  pairs4   four pairs over two arm sums -> one chunk, k_svr_dense<5>

Both strands are part of every grid."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "svr_dense_bits.json")
SAMPLE = 8                                   # words of the strided sample kept per array

pytestmark = pytest.mark.gpu

#        name        capture     overlap  pairs           regions (bed start, bed end)      n_sv  sv_split
CASES = [("wide_sv3", (140, 180), 30, slice(0, 57), [(3000, 3166), (5000, 5569)], 3, 1),
         ("wide_sv4", (140, 180), 30, slice(0, 57), [(3000, 3166), (5000, 5569)], 4, 1),
         ("wide_sv7", (140, 180), 30, slice(0, 57), [(3000, 3166), (5000, 5569)], 7, 1),
         ("wide_sv7_split2", (140, 180), 30, slice(0, 57), [(3000, 3166), (5000, 5569)], 7, 2),
         ("mid_sv7", (150, 170), 150, slice(0, 57), [(0, 56), (3000, 3180)], 7, 1),
         ("one_sv4", (150, 150), 30, slice(0, 57), [(7000, 7200)], 4, 1),
         ("pairs16_sv7", (140, 180), 30, slice(0, 16), [(3000, 3166)], 7, 1),
         ("pairs4_sv3", (140, 180), 30, slice(10, 14), [(3000, 3166)], 3, 1)]
EXPECT_POSITIONS = {"wide_sv3": [300, 703], "mid_sv7": [56, 304], "one_sv4": [304], "pairs16_sv7": [300]}


def _genome():
    from mipgen_amd import synth
    return synth.random_genome(12000, 11, n_run_frac=0.002, n_run_len=6)


def _run_case(case, tmpdir):
    """-> (positions per region, scores as int64 words, records) of one case, scored through the C ABI"""
    from mipgen_amd import capi, synth
    name, (cmin, cmax), overlap, sl, beds, n_sv, split = case
    genome = _genome()
    pairs = synth.arm_pairs_from_sums()[sl]
    P = capi.make_params(cmin, cmax, score_method=capi.SCORE_SVR, max_mip_overlap=overlap, arm_pairs=pairs)
    model = os.path.join(tmpdir, f"svr_bits_{n_sv}.model")
    if not os.path.exists(model):
        synth.synthetic_svr_model(model, genome, n_sv, seed=5)
    regions = [capi.build_region(genome, "1", b0, b1, P, bwa_mode="hashed", label=f"r{i}", lrc=np.linspace(0.01 + 0.1 * i, 0.3, 44))
               for i, (b0, b1) in enumerate(beds)]
    acc = capi.Accel(P, device=0)
    try:
        acc.load_model_file(model)
        acc.set_sv_split(split)
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
def test_scores_and_records_keep_every_bit(case, golden, tmp_path_factory):
    tmpdir = str(tmp_path_factory.getbasetemp())
    n_pos, words, records = _run_case(case, tmpdir)
    got, want = _summary(n_pos, words, records), golden[case[0]]
    if case[0] in EXPECT_POSITIONS:                                   # the grids are the ones whose tile shapes the docstring lists
        assert n_pos == EXPECT_POSITIONS[case[0]]
    assert got["positions"] == want["positions"]
    assert got["nan_scores"] == want["nan_scores"]
    for what in ("records", "scores"):
        g, w = got[what], want[what]
        assert g["n"] == w["n"]
        if g["sha256"] != w["sha256"]:
            diff = [(i, a, b) for i, a, b in zip(w["at"], g["words"], w["words"]) if a != b]
            pytest.fail(f"{case[0]}: {what} differ from the recording (sha256 {g['sha256'][:16]} != {w['sha256'][:16]}); sampled words that differ "
                        f"(index, got, recorded): {diff[:4] or 'none of the sample'}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_svr_bits.py --record   (rewrites tests/golden/svr_dense_bits.json from this build, on a GPU)")
    import tempfile
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for c in CASES:
            out[c[0]] = _summary(*_run_case(c, td))
            print(c[0], out[c[0]]["positions"], out[c[0]]["scores"]["n"], out[c[0]]["scores"]["sha256"][:16], "NaN", out[c[0]]["nan_scores"], flush=True)
    with open(os.environ.get("SVR_BITS_OUT", GOLDEN), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
