"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run - only the headline: K timed steps, `ms_per_step`, none of the --full lines - and
--dump-outputs, the last timed step's emitted counts and condensed survivors, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps_the_last_steps_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", a)
    assert line["metric"] == "candidate MIPs scored/sec (SVR)" and line["unit"] == "candidates/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["parity_checked"] is False and not {"exome_strong", "scale_base", "extra", "cpu_baseline"} & set(line)
    got = {f[:-4]: np.load(os.path.join(a, f)) for f in os.listdir(a)}
    assert sorted(got) == ["emitted", "survivor_cand_index", "survivor_record_hi", "survivor_record_lo", "survivor_score"]
    assert all(v.dtype == np.float64 for v in got.values())
    cfg = line["config"]
    assert got["emitted"].shape[0] == cfg["regions_rank0"] and int(got["emitted"].sum()) == cfg["emitted_candidates_rank0"]
    assert int((got["survivor_cand_index"] >= 0).sum()) == cfg["survivors_rank0"] > 0
    assert np.all(got["survivor_cand_index"] < cfg["dense_candidates_rank0"])
    # the same arguments (but other step counts): the same inputs, the same outputs
    _bench("--steps", "1", "--warmup", "0", "--dump-outputs", b)
    for name, v in got.items():
        assert np.array_equal(v, np.load(os.path.join(b, name + ".npy")), equal_nan=True), name
