"""CPU: the parts of SVR model selection that need no device - the ctypes mirrors of its C structs, libsvm's fold assignment
(mipgen_accel_svr_cv_folds against a restatement of svm.cpp:2408-2415 driven by libc's own srand / rand), and `mipgen_svr_cv`'s option and
data-file checks, which all run before the device is touched (so they exit 1 with a message here too), and its no-device error."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi

CV_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_svr_cv")
GOOD = "1.5 1:0.25 3:-1 192:4\n0.5 2:1e-3 5:0.5\n2.25 1:1 2:2 3:3\n1.0 4:1\n"


def run(args, cwd, data=GOOD):
    with open(os.path.join(cwd, "train.txt"), "w") as fh:
        fh.write(data)
    return subprocess.run([CV_BIN] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_struct_mirrors_match_the_header():
    assert C.sizeof(capi.SvrCvPoint) == 24
    assert C.sizeof(capi.SvrCvResult) == 32
    assert capi.SvrCvResult.iterations.offset == 16 and capi.SvrCvResult.n_sv_total.offset == 24
    for name in ("mipgen_accel_train_svr", "mipgen_accel_svr_cv_folds", "mipgen_accel_cross_validate_svr"):
        assert name in capi.EXPORTED_SYMBOLS
    assert hasattr(capi.Accel, "cross_validate_svr") and hasattr(capi, "svr_cv_folds")
    assert capi.load_library().mipgen_accel_abi_version() == 6          # additions only


def libsvm_folds(n, nr_fold, seed):
    """svm_cross_validation's regression branch (svm.cpp:2349-2353, 2408-2415) on the C library's own generator."""
    libc = C.CDLL("libc.so.6")
    libc.srand.argtypes = [C.c_uint]
    libc.rand.restype = C.c_int
    if nr_fold > n:
        nr_fold = n
    libc.srand(seed)
    perm = list(range(n))
    for i in range(n):
        j = i + libc.rand() % (n - i)
        perm[i], perm[j] = perm[j], perm[i]
    return perm, [i * n // nr_fold for i in range(nr_fold + 1)]


@pytest.mark.parametrize("seed", [1, 7, 12345])
@pytest.mark.parametrize("folds", [2, 5, 10, 50])
@pytest.mark.parametrize("n", [1, 7, 40, 1500])
def test_folds_are_libsvms(n, folds, seed):
    perm, start = capi.svr_cv_folds(n, folds, seed)
    want_perm, want_start = libsvm_folds(n, folds, seed)
    assert perm.tolist() == want_perm
    assert start.tolist() == want_start
    used = min(folds, n)
    assert sorted(perm.tolist()) == list(range(n))
    assert len(start) == used + 1 and all(start[i] == i * n // used for i in range(used + 1))


def test_folds_do_not_touch_the_process_stream_and_seed_0_is_seed_1():
    libc = C.CDLL("libc.so.6")
    libc.srand.argtypes = [C.c_uint]
    libc.srand(99)
    a = [libc.rand() for _ in range(3)]
    libc.srand(99)
    capi.svr_cv_folds(100, 5, 3)
    assert [libc.rand() for _ in range(3)] == a
    assert capi.svr_cv_folds(200, 5, 0)[0].tolist() == capi.svr_cv_folds(200, 5, 1)[0].tolist()
    assert capi.svr_cv_folds(200, 5, 1)[0].tolist() != capi.svr_cv_folds(200, 5, 7)[0].tolist()
    big = 2 ** 31 + 5                                                    # a seed above INT_MAX: srandom_r's arithmetic on a negative word
    assert capi.svr_cv_folds(300, 5, big)[0].tolist() == libsvm_folds(300, 5, big)[0]


def test_folds_refuse_nonsense():
    for n, folds in ((0, 5), (-1, 5), (10, 0), (10, -2)):
        with pytest.raises(capi.AccelError, match=r"error -1: \S"):
            capi.svr_cv_folds(n, folds, 1)


@pytest.mark.parametrize("args,needle", [
    (["-g", "0.1,x", "train.txt"], "bad list for -g"),
    (["-c", "1,,2", "train.txt"], "bad list for -c"),
    (["-p", "0.1,", "train.txt"], "bad list for -p"),
    (["-g", "", "train.txt"], "bad list for -g"),
    (["-c", "1,0", "train.txt"], "C <= 0"),
    (["-p", "0.1,-1", "train.txt"], "p < 0"),
    (["-g", "0.1,-0.5", "train.txt"], "gamma < 0"),
    (["-g", "nan", "train.txt"], "gamma < 0"),
    (["-e", "0", "train.txt"], "eps <= 0"),
    (["-e", "abc", "train.txt"], "bad value for -e"),
    (["-v", "1", "train.txt"], "n must >= 2"),
    (["-v", "0", "train.txt"], "n must >= 2"),
    (["-v", "abc", "train.txt"], "bad value for -v"),
    (["-v", "2.5", "train.txt"], "bad value for -v"),
    (["-seed", "-3", "train.txt"], "bad value for -seed"),
    (["-seed", "x", "train.txt"], "bad value for -seed"),
    (["-s", "3", "train.txt"], "unknown option"),
    (["-h", "1", "train.txt"], "unknown option"),
    (["-vv", "5", "train.txt"], "unknown option"),
    (["-", "train.txt"], "unknown option"),
    (["-c"], "needs a value"),
    ([], "no training file"),
    (["train.txt", "extra"], "too many arguments"),
    (["missing.txt"], "can't open input file"),
])
def test_cli_option_errors(args, needle, tmp_path):
    p = run(["-o", "out.model"] + args, str(tmp_path))
    assert p.returncode == 1
    assert needle in p.stderr.decode(), p.stderr.decode()
    assert p.stdout == b"" and not os.path.exists(tmp_path / "out.model")


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
    ("1 1:1\n", "at least two"),
])
def test_cli_data_file_errors(data, needle, tmp_path):
    p = run(["-o", "out.model", "train.txt"], str(tmp_path), data)
    assert p.returncode == 1
    err = p.stderr.decode()
    assert needle in err and err.startswith("mipgen_svr_cv: "), err
    assert p.stdout == b"" and not os.path.exists(tmp_path / "out.model")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_reports_the_no_device_error(tmp_path):
    p = run(["-g", "0.1,0.2", "-o", "out.model", "train.txt"], str(tmp_path))
    assert p.returncode == 1
    assert "no HIP device" in p.stderr.decode(), p.stderr.decode()
    assert p.stdout == b"" and not os.path.exists(tmp_path / "out.model")
