"""CPU: bench.py --dump-outputs writes what the timed path returned as float64 arrays - every value exact, at most 64 MB, and above that
a sample of the survivor rows that depends only on their count (two builds run with the same arguments write the same rows)."""
import os

import numpy as np

import bench
from mipgen_amd import capi


def _survivors(n, seed=1):
    rng = np.random.default_rng(seed)
    s = np.zeros(n, dtype=capi.SURVIVOR_DTYPE)
    s["cand_index"] = rng.integers(-1, 1 << 40, size=n)
    s["score"] = rng.normal(size=n)
    s["score"][::7] = np.nan
    s["record"] = rng.integers(0, np.iinfo(np.uint64).max, size=n, dtype=np.uint64, endpoint=True)
    return s


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_float64_and_exact(tmp_path):
    emitted = np.arange(5, dtype=np.int64) * 1000
    surv = _survivors(300)
    bench.dump_outputs(str(tmp_path), emitted, surv)
    got = _load(str(tmp_path))
    assert sorted(got) == ["emitted", "survivor_cand_index", "survivor_record_hi", "survivor_record_lo", "survivor_score"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["emitted"].astype(np.int64), emitted)
    assert np.array_equal(got["survivor_cand_index"].astype(np.int64), surv["cand_index"])
    assert np.array_equal(got["survivor_score"], surv["score"], equal_nan=True)
    rec = (got["survivor_record_hi"].astype(np.uint64) << np.uint64(32)) | got["survivor_record_lo"].astype(np.uint64)
    assert np.array_equal(rec, surv["record"])


def test_dump_above_the_cap_is_a_fixed_sample(tmp_path):
    emitted = np.ones(10, dtype=np.int64)
    surv = _survivors(20000)
    cap = 256 << 10
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), emitted, surv if d == "a" else _survivors(20000, seed=2), cap_bytes=cap)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= cap
    rows = a["survivor_rows"].astype(np.int64)
    assert 0 < rows.size < surv.shape[0] and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["survivor_rows"], b["survivor_rows"])          # the rows depend on the row count only
    assert np.array_equal(a["survivor_cand_index"].astype(np.int64), surv["cand_index"][rows])
    assert np.array_equal(a["survivor_score"], surv["score"][rows], equal_nan=True)
