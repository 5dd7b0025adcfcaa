"""The kernels of kernels_svr_train.hip reached from Python, one launcher at a time (tests/test_gpu_svt_kernels.py): ctypes mirrors of SvtCtl, SvtProb and
SvtPred (svr_train.h asserts their sizes, tests/test_svr_train_cpu.py the mirrors'), the eight mipgen_svt_launch_* functions - exported as every symbol of the
library is - and device memory as torch tensors whose data_ptr() goes into the descriptors.  Launches go on the null stream and are followed by
torch.cuda.synchronize().  Every array a kernel reads or writes lies between two guards of GUARD elements of a sentinel byte, and every launch is followed by a
check that all guards of the batch are untouched.  torch starts first, then the library: Device() is made in a process that has not touched the library."""
import ctypes as C

import numpy as np

from tests import svt_ref as R

GUARD = 64                 # elements on either side of every array
SENTINEL = 0xA5


class SvtCtl(C.Structure):
    _fields_ = [("iter", C.c_int64), ("max_iter", C.c_int64), ("active", C.c_int32), ("counter", C.c_int32), ("after_recon", C.c_int32),
                ("exit_code", C.c_int32), ("n_free", C.c_int32), ("pad", C.c_int32), ("gmax1", C.c_double), ("gmax2", C.c_double)]


class SvtProb(C.Structure):
    _fields_ = [("n", C.c_int32), ("ldk", C.c_int32), ("rows", C.c_void_p), ("K", C.c_void_p), ("qd", C.c_void_p), ("lin", C.c_void_p),
                ("perm", C.c_void_p), ("G", C.c_void_p), ("Gbar", C.c_void_p), ("alpha", C.c_void_p), ("st", C.c_void_p), ("ctl", C.c_void_p),
                ("flag", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p), ("fperm", C.c_void_p), ("falpha", C.c_void_p),
                ("C", C.c_double), ("eps", C.c_double)]


class SvtPred(C.Structure):
    _fields_ = [("n_sv", C.c_int32), ("n_held", C.c_int32), ("sv_rows", C.c_void_p), ("coef", C.c_void_p), ("held", C.c_void_p), ("out", C.c_void_p),
                ("gamma", C.c_double), ("rho", C.c_double)]


_p, _i, _d = C.c_void_p, C.c_int, C.c_double
LAUNCHERS = {
    "gram": [_p, _i, _d, _p, _p, _p, _p],                     # stream, n, gamma, x, xsq, qd, K
    "init": [_p, _p, _p, _i, _i],                             # stream, probs, list, count, max_n
    "iterate": [_p, _p, _p, _i, _i],
    "shrink_stats": [_p, _p, _p, _i],
    "shrink": [_p, _p, _p, _i],
    "free_list": [_p, _p, _p, _i],
    "reconstruct": [_p, _p, _p, _i, _i],                      # ..., max_inactive
    "predict": [_p, _p, _p, _i, _i],                          # stream, x, preds, count, max_held
}


def bind(lib):
    for name, args in LAUNCHERS.items():
        fn = getattr(lib, "mipgen_svt_launch_" + name)
        fn.argtypes = args
        fn.restype = C.c_int
    return lib


def ctl_struct(d) -> SvtCtl:
    return SvtCtl(**{k: d[k] for k in R.State.CTL})


def ctl_dict(raw: bytes) -> dict:
    c = SvtCtl.from_buffer_copy(raw)
    return {k: getattr(c, k) for k in R.State.CTL}


class DeviceTrouble(Exception):
    """a launch failed, the device reported an error or a guard was written: nothing more is to be launched in this process"""


class Device:
    """torch first, then the library; one per process"""

    def __init__(self):
        import torch
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda:0")
        torch.cuda.synchronize()
        from mipgen_amd import capi
        self.torch = torch
        self.lib = bind(C.CDLL(capi.LIB_PATH))
        self.bufs = []

    def buf(self, arr):
        b = Buf(self, arr)
        self.bufs.append(b)
        return b

    def launch(self, name, *args):
        """one launcher on the null stream, synchronised; then every guard made so far is checked"""
        rc = getattr(self.lib, "mipgen_svt_launch_" + name)(None, *args)
        try:
            self.torch.cuda.synchronize()
        except RuntimeError as e:
            raise DeviceTrouble(f"mipgen_svt_launch_{name}: {e}") from e
        if rc != 0:
            raise DeviceTrouble(f"mipgen_svt_launch_{name}: hipError_t {rc}")
        for b in self.bufs:
            b.check(f"after {name}")

    def release(self):
        self.bufs = []


class Buf:
    """a host array on the device between two guards"""

    def __init__(self, dev: Device, arr):
        arr = np.ascontiguousarray(arr)
        self.dev, self.dtype, self.shape, self.nbytes = dev, arr.dtype, arr.shape, arr.nbytes
        self.g = GUARD * arr.dtype.itemsize
        host = np.full(self.g + self.nbytes + self.g, SENTINEL, dtype=np.uint8)
        host[self.g:self.g + self.nbytes] = arr.reshape(-1).view(np.uint8)
        self.t = dev.torch.from_numpy(host).to("cuda:0")
        self.ptr = self.t.data_ptr() + self.g
        assert self.ptr % arr.dtype.itemsize == 0

    def put(self, arr):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.shape == self.shape
        self.t[self.g:self.g + self.nbytes] = self.dev.torch.from_numpy(arr.reshape(-1).view(np.uint8).copy()).to("cuda:0")

    def raw(self):
        return self.t.cpu().numpy()

    def check(self, when=""):
        ok = bool((self.t[:self.g] == SENTINEL).all().item()) and bool((self.t[self.g + self.nbytes:] == SENTINEL).all().item())
        if not ok:
            raise DeviceTrouble(f"a guard of a {self.dtype} array of shape {self.shape} was written {when}")

    def get(self):
        return self.raw()[self.g:self.g + self.nbytes].copy().view(self.dtype).reshape(self.shape)


class DevProblem:
    """One SvtProb: the device arrays of a svt_ref.State.  K and qd may be shared between problems (pass their Bufs)."""
    SCRATCH = (("flag", np.int8), ("lo", np.int32), ("hi", np.int32), ("fperm", np.int32), ("falpha", np.float64))

    def __init__(self, dev: Device, s: R.State, K=None, qd=None):
        L = 2 * s.n
        self.dev, self.n, self.L = dev, s.n, L
        self.K = K if K is not None else dev.buf(s.K)
        self.qd = qd if qd is not None else dev.buf(s.qd)
        self.rows, self.lin = dev.buf(s.rows), dev.buf(s.lin)
        self.arrays = {name: dev.buf(getattr(s, name)) for name in R.State.ARRAYS}
        self.scratch = {name: dev.buf(np.zeros(L, dtype=dt)) for name, dt in self.SCRATCH}
        self.ctl = dev.buf(np.frombuffer(bytes(ctl_struct(s.ctl)), dtype=np.uint8))
        a, sc = self.arrays, self.scratch
        self.desc = SvtProb(n=s.n, ldk=s.ldk, rows=self.rows.ptr, K=self.K.ptr, qd=self.qd.ptr, lin=self.lin.ptr, perm=a["perm"].ptr, G=a["G"].ptr,
                            Gbar=a["Gbar"].ptr, alpha=a["alpha"].ptr, st=a["st"].ptr, ctl=self.ctl.ptr, flag=sc["flag"].ptr, lo=sc["lo"].ptr,
                            hi=sc["hi"].ptr, fperm=sc["fperm"].ptr, falpha=sc["falpha"].ptr, C=s.C, eps=s.eps)

    def upload(self, s: R.State):
        for name in R.State.ARRAYS:
            self.arrays[name].put(getattr(s, name))
        self.ctl.put(np.frombuffer(bytes(ctl_struct(s.ctl)), dtype=np.uint8))

    def download(self):
        out = {name: b.get() for name, b in self.arrays.items()}
        out["ctl"] = ctl_dict(self.ctl.get().tobytes())
        out["fperm"], out["falpha"] = self.scratch["fperm"].get(), self.scratch["falpha"].get()
        return out


class Batch:
    """The descriptor array of some problems and a launch list over it: `order` are indices into `problems`, workgroup b works on problems[order[b]]"""

    def __init__(self, dev: Device, problems, order=None):
        self.dev, self.problems = dev, list(problems)
        self.order = list(range(len(self.problems))) if order is None else list(order)
        self.descs = dev.buf(np.frombuffer(b"".join(bytes(p.desc) for p in self.problems), dtype=np.uint8))
        self.list = dev.buf(np.array(self.order, dtype=np.int32))
        self.max_n = max(self.problems[k].n for k in self.order)

    def launch(self, name, *extra):
        self.dev.launch(name, self.descs.ptr, self.list.ptr, len(self.order), *extra)


def state_bytes(s: R.State):
    """what a comparison looks at: the bytes of the five per-position arrays over all 2n positions and every field of the control block"""
    out = {name: np.ascontiguousarray(getattr(s, name)).tobytes() for name in R.State.ARRAYS}
    out["ctl"] = bytes(ctl_struct(s.ctl))
    return out


def assert_same_state(got: dict, want: R.State, what: str):
    """exact equality of the bytes of perm, G, Gbar, alpha and st over all 2n positions and of every field of SvtCtl"""
    for name in R.State.ARRAYS:
        w = np.ascontiguousarray(getattr(want, name))
        g = got[name]
        if g.tobytes() != w.tobytes():
            bad = np.nonzero(g.view(np.uint8).reshape(len(w), -1) != w.view(np.uint8).reshape(len(w), -1))[0]
            k = int(bad[0])
            raise AssertionError(f"{what}: {name} differs at {len(set(bad.tolist()))} of {len(w)} positions, first at {k}: device {g[k]!r}, model {w[k]!r}")
    wc = ctl_dict(bytes(ctl_struct(want.ctl)))
    gc = got["ctl"]
    diff = {k: (gc[k], wc[k]) for k in R.State.CTL if np.array(gc[k]).tobytes() != np.array(wc[k]).tobytes()}
    assert not diff, f"{what}: SvtCtl differs (device, model): {diff}"
