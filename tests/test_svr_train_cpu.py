"""CPU: the parts of the SVR trainer that need no device - the ctypes mirrors of its C structs, and `mipgen_svr_train`'s option and data-file
checks, which all run before the device is touched (so they exit 1 with a message here too), and its no-device error."""
import ctypes as C
import os
import subprocess

import pytest

from mipgen_amd import capi
from tests import svt_driver

TRAIN_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_svr_train")
GOOD = "1.5 1:0.25 3:-1 192:4\n0.5 2:1e-3 5:0.5\n2.25 1:1 2:2 3:3\n"


def run(args, cwd, data=GOOD):
    with open(os.path.join(cwd, "train.txt"), "w") as fh:
        fh.write(data)
    return subprocess.run([TRAIN_BIN] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_struct_mirrors_match_the_header():
    assert C.sizeof(capi.SvrTrainParams) == 40
    assert C.sizeof(capi.SvrTrainInfo) == 56
    assert capi.SvrTrainInfo.rho.offset == 16 and capi.SvrTrainInfo.n_shrink.offset == 32 and capi.SvrTrainInfo.solve_ms.offset == 48
    assert "mipgen_accel_train_svr" in capi.EXPORTED_SYMBOLS
    assert hasattr(capi.Accel, "train_svr")


def test_kernel_struct_mirrors_match_the_header():
    """svr_train.h static_asserts the same three sizes"""
    assert C.sizeof(svt_driver.SvtCtl) == 56 and C.sizeof(svt_driver.SvtProb) == 144 and C.sizeof(svt_driver.SvtPred) == 56
    assert svt_driver.SvtCtl.gmax1.offset == 40 and svt_driver.SvtProb.C.offset == 128 and svt_driver.SvtPred.gamma.offset == 40


@pytest.mark.parametrize("args,needle", [
    (["-s", "0", "train.txt"], "only -s 3"),
    (["-s", "4", "train.txt"], "only -s 3"),
    (["-t", "0", "train.txt"], "only -t 2"),
    (["-t", "3", "train.txt"], "only -t 2"),
    (["-h", "0", "train.txt"], "only -h 1"),
    (["-c", "0", "train.txt"], "C <= 0"),
    (["-p", "-1", "train.txt"], "p < 0"),
    (["-e", "0", "train.txt"], "eps <= 0"),
    (["-g", "-0.5", "train.txt"], "gamma < 0"),
    (["-g", "abc", "train.txt"], "bad value for -g"),
    (["-v", "5", "train.txt"], "unknown option"),
    (["-c"], "needs a value"),
    ([], "no training file"),
    (["train.txt", "a.model", "extra"], "too many arguments"),
    (["missing.txt"], "can't open input file"),
])
def test_cli_option_errors(args, needle, tmp_path):
    p = run(args, str(tmp_path))
    assert p.returncode == 1
    assert needle in p.stderr.decode(), p.stderr.decode()
    assert not os.path.exists(tmp_path / "train.txt.model")


@pytest.mark.parametrize("data,needle", [
    ("1 3:1 2:1\n", "indices must ascend"),
    ("1 2:1 2:1\n", "indices must ascend"),
    ("1 193:1\n", "above 192"),
    ("1 0:1\n", "indices must ascend"),
    ("1 1:nan\n", "not finite"),
    ("1 1:inf\n", "not finite"),
    ("nan 1:1\n", "label"),
    ("abc 1:1\n", "label"),
    ("1 1:x\n", "bad value"),
    ("1 a:1\n", "bad index"),
    ("1 1:1\n\n2 1:2\n", "empty line"),
    ("", "no training rows"),
])
def test_cli_data_file_errors(data, needle, tmp_path):
    p = run(["train.txt"], str(tmp_path), data)
    assert p.returncode == 1
    assert needle in p.stderr.decode(), p.stderr.decode()
    assert not os.path.exists(tmp_path / "train.txt.model")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_reports_the_no_device_error(tmp_path):
    p = run(["-q", "train.txt"], str(tmp_path))
    assert p.returncode == 1
    assert "no HIP device" in p.stderr.decode(), p.stderr.decode()
    assert not os.path.exists(tmp_path / "train.txt.model")
