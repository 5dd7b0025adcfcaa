"""GPU: every kernel of kernels_svr_train.hip alone, launched through its own mipgen_svt_launch_* function (tests/svt_driver.py) and held against the plain
sequential model of its contract (tests/svt_ref.py) at the shapes where lanes, wavefronts, strided rounds, prefix sums and tiles can go wrong.  Every comparison
is exact equality of the bytes of whole arrays: perm, G, Gbar, alpha and st over all 2n positions, every field of SvtCtl, and K, xsq, qd, out.  Rows are 192
random features in [0, 1] unless a case says otherwise; no reference build is needed.

The driver starts torch before the library, and this process may already hold the library's HIP runtime: so all cases run in ONE child process (this file run
as a module), each under its own time limit, and every test here looks up its case's verdict.  The child stops launching at the first sign of trouble on the
device (a failed launch, an error at synchronisation, a written guard); the cases it did not reach then fail with that report."""
import faulthandler
import json
import os
import subprocess
import sys
import time
import traceback

import numpy as np
import pytest

from tests import svt_driver as D
from tests import svt_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_LIMIT = 120           # seconds per case in the child; a case takes a second or two
GAMMAS = {"g0": 0.0, "g192th": 1 / 192, "g50": 50.0}
CASES = {}


def case(name):
    def reg(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return reg


def features(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, R.NF))


def input_matrix(m, seed, gamma=1 / 192):
    """a symmetric float matrix of RBF values over m random rows and its diagonal in double: an INPUT of the solver kernels, which take K as it comes (the
    Gram kernel has cases of its own), so numpy's exp will do"""
    x = features(m, seed)
    sq = (x * x).sum(axis=1)
    K = np.exp(-gamma * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0)).astype(np.float32)
    K = np.minimum(K, K.T)
    np.fill_diagonal(K, 1.0)
    return K, np.ones(m)


def labels(n, seed):
    return 1.4 + 1.1 * np.random.default_rng(seed).standard_normal(n)


def problem(n, seed, C=4.0, p=0.05, eps=1e-3, extra=0, y=None, K=None):
    """the state Solve starts from for n rows; extra > 0: a sub-problem, n shuffled rows of a matrix of order n + extra"""
    m = n + extra
    Kq = input_matrix(m, seed) if K is None else (K, np.ones(m))
    rows = np.random.default_rng(seed + 1).permutation(m)[:n] if extra else np.arange(n)
    y = labels(n, seed + 2) if y is None else np.asarray(y, dtype=np.float64)
    return R.init(R.State(Kq[0], Kq[1], rows, np.concatenate([p - y, p + y]), C, eps))


# ---- Gram ----------------------------------------------------------------------------------------------------------------------------------------
def gram_case(n, gname, variant):
    def run(dev):
        x = features(n, 1000 + n)
        if variant == "zeros":
            x[[0, n - 1]] = 0.0                               # two all-zero rows (one where n = 1)
        elif variant == "same":
            x[n - 1] = x[0]                                   # two identical rows
        gamma = GAMMAS[gname]
        bx, bxsq, bqd, bK = dev.buf(x), dev.buf(np.zeros(n)), dev.buf(np.zeros(n)), dev.buf(np.zeros((n, n), dtype=np.float32))
        dev.launch("gram", n, gamma, bx.ptr, bxsq.ptr, bqd.ptr, bK.ptr)
        xsq, qd, K = R.gram(x, gamma)
        gK = bK.get()
        assert bxsq.get().tobytes() == xsq.tobytes(), "xsq"
        assert bqd.get().tobytes() == qd.tobytes() and np.all(bqd.get() == 1.0), "qd"
        bad = np.argwhere(gK.view(np.uint32) != K.view(np.uint32))
        assert bad.size == 0, f"K differs at {len(bad)} entries, first {bad[0]}: device {gK[tuple(bad[0])]!r}, model {K[tuple(bad[0])]!r}"
        assert np.array_equal(gK, gK.T), "K is not symmetric"
        if gname == "g50" and variant == "plain":
            assert np.count_nonzero(gK) == n                  # every argument off the diagonal lies below -110
    return run


for _n in (1, 15, 16, 17, 33, 49):
    for _g in GAMMAS:
        for _v in ("plain", "zeros", "same"):
            CASES[f"gram-n{_n}-{_g}-{_v}"] = gram_case(_n, _g, _v)


# ---- the iteration loop --------------------------------------------------------------------------------------------------------------------------
def both_routes(dev, s0: R.State, what, limit=64):
    """One launch from s0 through k_svt_iterate<true> (max_n = n) and through k_svt_iterate<false> (max_n = SVT_LDS_ROW + 1): both must leave the
    model's state.  Returns the model's state."""
    want = R.iterate(s0.copy(), n_launch_limit=limit)
    P = D.DevProblem(dev, s0)
    B = D.Batch(dev, [P])
    for route, max_n in (("LDS", s0.n), ("global", R.LDS_ROW + 1)):
        P.upload(s0)
        B.launch("iterate", max_n)
        D.assert_same_state(P.download(), want, f"{what}, {route} route")
    dev.release()
    return want


def counter_case(n, counter):
    def run(dev):
        s = problem(n, 2000 + n)
        if counter > 1:                                       # from the middle of a solve (free and bounded variables of both signs), the model's
            s.ctl["counter"] = min(n // 2, 40)
            R.iterate(s, n_launch_limit=40)
        it0 = s.ctl["iter"]
        s.ctl["counter"] = counter
        want = both_routes(dev, s, f"n {n}, counter {counter}")
        if n >= 31:
            assert np.count_nonzero(s.st != R.LOWER) >= (counter > 1) * 10
            assert want.ctl["exit_code"] == R.EXIT_SHRINK and want.ctl["iter"] == it0 + counter and want.ctl["counter"] == min(2 * n, 1000), want.ctl
        if n == 1:                                            # one row: its two variables cannot both move, optimal at once
            assert want.ctl["exit_code"] == R.EXIT_OPTIMAL and want.ctl["iter"] == 0
    return run


for _n in (1, 2, 31, 32, 33, 511, 512, 513, 1100):
    for _c in (1, 2, 7):
        CASES[f"iterate-n{_n}-counter{_c}"] = counter_case(_n, _c)


def to_the_end_case(n):
    def run(dev):
        s = problem(n, 2100 + n, C=20.0, p=0.05, eps=1e-5)
        s.ctl["counter"] = 1000                               # no shrinking point on the way
        s = both_routes(dev, s, f"n {n} to the optimum", limit=900)
        assert s.ctl["exit_code"] == R.EXIT_OPTIMAL and s.ctl["iter"] > 0, s.ctl
        s.ctl["after_recon"] = 1                              # the re-check after reconstruct_gradient: optimal again, nothing moves
        t = both_routes(dev, s, f"n {n} re-check")
        assert t.ctl["exit_code"] == R.EXIT_DONE and t.ctl["iter"] == s.ctl["iter"] and t.ctl["after_recon"] == 1
        if n == 2:                                            # optimal before a third iteration
            return
        u = problem(n, 2100 + n, C=20.0, p=0.05, eps=1e-5)
        u.ctl["iter"] = 41
        u.ctl["max_iter"] = 44
        u = both_routes(dev, u, f"n {n} to max_iter")
        assert u.ctl["exit_code"] == R.EXIT_MAXITER and u.ctl["iter"] == 44, u.ctl
        v = problem(n, 2100 + n, C=20.0, p=0.05, eps=1e-5)                # the re-check finds work: counter = 1, so the launch ends after that one iteration
        v.ctl["after_recon"] = 1
        v = both_routes(dev, v, f"n {n} re-check with work left")
        assert v.ctl["exit_code"] == R.EXIT_SHRINK and v.ctl["iter"] == 1 and v.ctl["after_recon"] == 0, v.ctl
    return run


for _n in (2, 17, 33):
    CASES[f"iterate-n{_n}-to-the-end"] = to_the_end_case(_n)


def empty_up_set_case(n):
    def run(dev):
        s = problem(n, 2200 + n)
        rng = np.random.default_rng(n)
        s.alpha[:n] = s.C
        s.st[:n] = R.UPPER
        s.G = rng.standard_normal(2 * n)
        before = D.state_bytes(s)
        want = both_routes(dev, s, f"n {n}, empty up-set")
        assert want.ctl["exit_code"] == R.EXIT_OPTIMAL and want.ctl["iter"] == 0
        after = D.state_bytes(want)
        assert all(after[k] == before[k] for k in R.State.ARRAYS)
    return run


for _n in (33, 600):
    CASES[f"iterate-n{_n}-empty-up-set"] = empty_up_set_case(_n)


def tie_case(n, same_rows):
    """Every candidate of the first argmax equal, over every lane and wavefront: the linear term is -1 at every y = +1 position and -3 at every y = -1
    position, all at their lower bound, so I_up is the y = +1 half with -G = 1 everywhere and position n - 1 must win.  With identical rows as well K is 1
    everywhere: the quad_coef of every y = -1 partner is 0 (the SVT_TAU branch), every obj_diff is -16 / tau, and position 2n - 1 must win the argmin."""
    def run(dev):
        K = np.ones((n, n), dtype=np.float32) if same_rows else None
        s = problem(n, 2300 + n, K=K)
        s.lin = np.concatenate([np.full(n, -1.0), np.full(n, -3.0)])
        R.init(s)
        s.ctl["counter"] = 1
        want = both_routes(dev, s, f"n {n}, ties" + (", identical rows" if same_rows else ""))
        moved = np.nonzero(want.alpha)[0]
        assert want.ctl["iter"] == 1 and moved.size == 2 and moved[0] == n - 1, moved
        if same_rows:
            assert moved[1] == 2 * n - 1 and want.alpha[n - 1] == s.C and want.alpha[2 * n - 1] == s.C, (moved, want.alpha[moved])
    return run


for _n in (33, 512, 1100):
    CASES[f"iterate-n{_n}-ties"] = tie_case(_n, False)
    CASES[f"iterate-n{_n}-ties-identical-rows"] = tie_case(_n, True)


def shuffled_state_case(n):
    """Any state is an input: positions in a random order (the two signs interleaved, as after shrinking), a third of them each lower, upper and free, a
    random gradient, the last 37 inactive.  Both branches of the second loop have candidates on every lane."""
    def run(dev):
        s = problem(n, 2350 + n)
        t = random_state(n, 2 * n - 37, 2360 + n)
        for name in R.State.ARRAYS:
            setattr(s, name, getattr(t, name))
        s.ctl["active"] = 2 * n - 37
        s.ctl["counter"] = 7
        want = both_routes(dev, s, f"n {n}, shuffled state")
        assert want.ctl["exit_code"] == R.EXIT_SHRINK and want.ctl["iter"] == 7
    return run


for _n in (33, 512, 1100):
    CASES[f"iterate-n{_n}-shuffled-state"] = shuffled_state_case(_n)


def sub_problem_case(n):
    def run(dev):
        s = problem(n, 2400 + n, extra=9)
        assert s.ldk == n + 9 and not np.array_equal(s.rows, np.arange(n))
        s.ctl["counter"] = 7
        both_routes(dev, s, f"n {n} of {n + 9} rows")
    return run


for _n in (33, 513):
    CASES[f"iterate-n{_n}-sub-problem"] = sub_problem_case(_n)


def bound_case(n):
    """C so small that the first step ends at the bound: the status change writes G_bar over all 2n positions while G moves only below `active`"""
    def run(dev):
        s = problem(n, 2500 + n, C=1e-3)
        A = 2 * n - 70 if n > 40 else 2 * n - 5
        s.ctl["active"] = A
        s.ctl["counter"] = 2
        want = both_routes(dev, s, f"n {n}, active {A}, C 1e-3")
        assert np.count_nonzero(want.st == R.UPPER) >= 2 and np.all(want.Gbar[A:] != 0) and np.array_equal(want.G[A:], s.G[A:])
    return run


for _n in (33, 600):
    CASES[f"iterate-n{_n}-status-change"] = bound_case(_n)


# ---- do_shrinking ----------------------------------------------------------------------------------------------------------------------------------
def random_state(n, A, seed):
    """any state of 2n positions with A of them active: the shrinking and reconstruction kernels read no K below the active size"""
    rng = np.random.default_rng(seed)
    L = 2 * n
    s = R.State(np.ones((1, 1), dtype=np.float32), np.ones(1), np.zeros(n, dtype=np.int32), rng.standard_normal(L), 4.0, 1e-3)
    s.perm = rng.permutation(L).astype(np.int32)
    s.G = rng.standard_normal(L)
    s.Gbar = rng.standard_normal(L)
    s.st = rng.integers(0, 3, L).astype(np.int8)
    s.alpha = np.where(s.st == R.UPPER, s.C, np.where(s.st == R.LOWER, 0.0, rng.uniform(0.1, 3.9, L)))
    s.ctl["active"] = A
    return s


def plant_flags(s: R.State, flags, rng):
    """G and st such that, with gmax1 = gmax2 = 0, be_shrunk is `flags` over the active positions: shrunk is a bound position whose gradient points
    outward (lower bound with G > 0, upper bound with G < 0), kept is a free one or a bound one whose gradient points inward"""
    A = len(flags)
    mag = rng.uniform(0.5, 2.0, A)
    pick = rng.integers(0, 3, A)
    st = np.where(flags, np.where(pick == 0, R.UPPER, R.LOWER), np.where(pick == 0, R.FREE, np.where(pick == 1, R.LOWER, R.UPPER)))
    outward = np.where(st == R.LOWER, mag, -mag)
    s.st[:A] = st
    s.G[:A] = np.where(flags, outward, np.where(st == R.FREE, rng.standard_normal(A), -outward))
    s.ctl["gmax1"] = s.ctl["gmax2"] = 0.0


def flag_patterns(A, rng):
    k = np.arange(A)
    one_chunk = np.zeros(A, dtype=bool)
    one_chunk[[max(A - 3, 0), A - 1]] = True                  # the one swap pairs two positions of the last thread's chunk
    return {"none": k < 0, "all": k >= 0, "lower-half": k < A // 2, "upper-half": k >= A // 2, "alternating": k % 2 == 0, "only-0": k == 0,
            "only-last": k == A - 1, "one-chunk": one_chunk, "tenth": rng.random(A) < 0.1, "half": rng.random(A) < 0.5, "most": rng.random(A) < 0.9}


def shrink_case(A, full):
    def run(dev):
        n = A // 2 if full else A // 2 + 41
        rng = np.random.default_rng(3000 + A)
        s = random_state(n, A, 3100 + A)
        P = D.DevProblem(dev, s)
        B = D.Batch(dev, [P])
        # the statistics of a random state, then do_shrinking with them
        P.upload(s)
        B.launch("shrink_stats")
        want = s.copy()
        R.shrink_stats(want)
        D.assert_same_state(P.download(), want, f"A {A}: shrink_stats")
        B.launch("shrink")
        R.shrink(want)
        D.assert_same_state(P.download(), want, f"A {A}: shrink after shrink_stats")
        for name, flags in flag_patterns(A, rng).items():
            t = s.copy()
            plant_flags(t, flags, rng)
            assert [R.be_shrunk(t, k) for k in range(A)] == flags.tolist()
            P.upload(t)
            B.launch("shrink")
            R.shrink(t)
            assert t.ctl["active"] == A - int(flags.sum())
            D.assert_same_state(P.download(), t, f"A {A}, pattern {name}")
    return run


for _A in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 3000):
    if _A % 2 == 0:
        CASES[f"shrink-A{_A}-all-active"] = shrink_case(_A, True)
    CASES[f"shrink-A{_A}-some-inactive"] = shrink_case(_A, False)


# ---- reconstruct_gradient ------------------------------------------------------------------------------------------------------------------------
def recon_state(n, inactive, n_free, seed, extra=9):
    rng = np.random.default_rng(seed)
    L, A = 2 * n, 2 * n - inactive
    assert 0 < A and n_free <= A
    s = problem(n, seed, extra=extra)
    s.perm = rng.permutation(L).astype(np.int32)
    s.G = rng.standard_normal(L)
    s.Gbar = rng.standard_normal(L)
    s.st = rng.integers(0, 2, L).astype(np.int8)
    s.st[rng.choice(A, n_free, replace=False)] = R.FREE
    s.st[A:][rng.random(inactive) < 0.3] = R.FREE           # free positions above the active size are not listed
    s.alpha = np.where(s.st == R.UPPER, s.C, np.where(s.st == R.LOWER, 0.0, rng.uniform(0.1, 3.9, L)))
    s.ctl["active"] = A
    s.ctl["n_free"] = -7                                      # free_list writes it
    return s


def recon_case(n_free, inactive):
    def run(dev):
        n = 700
        s = recon_state(n, inactive, n_free, 4000 + 10 * n_free + inactive)
        P = D.DevProblem(dev, s)
        B = D.Batch(dev, [P])
        B.launch("free_list")
        want = R.free_list(s.copy())
        got = P.download()
        assert want.ctl["n_free"] == n_free
        D.assert_same_state(got, want, f"n_free {n_free}: free_list")
        assert got["fperm"][:n_free].tobytes() == want.fperm.tobytes() and got["falpha"][:n_free].tobytes() == want.falpha.tobytes(), "the free list"
        B.launch("reconstruct", inactive)
        R.reconstruct(want)
        D.assert_same_state(P.download(), want, f"n_free {n_free}, {inactive} inactive: reconstruct")
        assert np.array_equal(want.G[:2 * n - inactive], s.G[:2 * n - inactive]) and (n_free == 0 or not np.array_equal(want.G, s.G))
    return run


for _f in (0, 1, 17, 1025):
    for _i in (1, 255, 256, 257):
        CASES[f"reconstruct-free{_f}-inactive{_i}"] = recon_case(_f, _i)


# ---- batches: three problems of different n in one launch, listed in another order than the descriptors ------------------------------------------
ORDER = [2, 0, 1]


@case("batch-iterate")
def batch_iterate(dev):
    states = [problem(n, 5000 + n, extra=e) for n, e in ((33, 0), (513, 9), (100, 3))]
    for s, c in zip(states, (7, 2, 5)):
        s.ctl["counter"] = c
    want = [R.iterate(s.copy(), n_launch_limit=8) for s in states]
    Ps = [D.DevProblem(dev, s) for s in states]
    B = D.Batch(dev, Ps, ORDER)
    for route, max_n in (("LDS", B.max_n), ("global", R.LDS_ROW + 1)):
        for P, s in zip(Ps, states):
            P.upload(s)
        B.launch("iterate", max_n)
        for k, (P, w) in enumerate(zip(Ps, want)):
            D.assert_same_state(P.download(), w, f"problem {k} of the batch, {route} route")


@case("batch-init")
def batch_init(dev):
    states = [problem(n, 5100 + n) for n in (1, 513, 100)]
    Ps = []
    for s in states:
        junk = random_state(s.n, 2 * s.n, 5150 + s.n)
        junk.K, junk.qd, junk.rows, junk.ldk, junk.lin, junk.ctl = s.K, s.qd, s.rows, s.ldk, s.lin, dict(s.ctl)
        Ps.append(D.DevProblem(dev, junk))
    B = D.Batch(dev, Ps, ORDER)
    B.launch("init", B.max_n)
    for k, (P, s) in enumerate(zip(Ps, states)):
        D.assert_same_state(P.download(), s, f"problem {k} of the batch: init")


@case("batch-shrink")
def batch_shrink(dev):
    states = [random_state(n, A, 5200 + n) for n, A in ((33, 66), (1500, 2049), (100, 130))]
    Ps = [D.DevProblem(dev, s) for s in states]
    B = D.Batch(dev, Ps, ORDER)
    B.launch("shrink_stats")
    want = [s.copy() for s in states]
    for k, (P, w) in enumerate(zip(Ps, want)):
        R.shrink_stats(w)
        D.assert_same_state(P.download(), w, f"problem {k} of the batch: shrink_stats")
    B.launch("shrink")
    for k, (P, w) in enumerate(zip(Ps, want)):
        R.shrink(w)
        D.assert_same_state(P.download(), w, f"problem {k} of the batch: shrink")


@case("batch-reconstruct")
def batch_reconstruct(dev):
    shapes = ((33, 5, 17), (700, 257, 1025), (100, 60, 1))    # n, inactive, n_free
    states = [recon_state(n, i, f, 5300 + n, extra=e) for (n, i, f), e in zip(shapes, (0, 9, 3))]
    Ps = [D.DevProblem(dev, s) for s in states]
    B = D.Batch(dev, Ps, ORDER)
    B.launch("free_list")
    want = [R.free_list(s.copy()) for s in states]
    B.launch("reconstruct", max(i for _, i, _ in shapes))
    for k, (P, w) in enumerate(zip(Ps, want)):
        got = P.download()
        f = w.ctl["n_free"]
        assert got["fperm"][:f].tobytes() == w.fperm.tobytes() and got["falpha"][:f].tobytes() == w.falpha.tobytes(), f"problem {k}: the free list"
        D.assert_same_state(got, R.reconstruct(w), f"problem {k} of the batch: reconstruct")


# ---- predict -------------------------------------------------------------------------------------------------------------------------------------
def pred_desc(dev, sv_rows, coef, held, out_buf, gamma, rho):
    bs, bc, bh = dev.buf(np.asarray(sv_rows, dtype=np.int32)), dev.buf(np.asarray(coef, dtype=np.float64)), dev.buf(np.asarray(held, dtype=np.int32))
    return D.SvtPred(n_sv=len(sv_rows), n_held=len(held), sv_rows=bs.ptr, coef=bc.ptr, held=bh.ptr, out=out_buf.ptr, gamma=gamma, rho=rho)


def launch_predict(dev, bx, descs):
    bd = dev.buf(np.frombuffer(b"".join(bytes(d) for d in descs), dtype=np.uint8))
    dev.launch("predict", bx.ptr, bd.ptr, len(descs), max(d.n_held for d in descs))


def predict_case(n_sv, n_held):
    def run(dev):
        m = 120
        rng = np.random.default_rng(6000 + 100 * n_sv + n_held)
        x = features(m, 6001)
        x[3] = 0.0
        pick = rng.permutation(m)
        held, sv_rows = pick[:n_held], np.sort(pick[40:40 + n_sv])
        coef, rho, gamma = rng.uniform(-4.0, 4.0, n_sv), float(rng.uniform(-2, 2)), 1 / 192
        out0 = 1000.0 + np.arange(m)
        bx, bout = dev.buf(x), dev.buf(out0)
        launch_predict(dev, bx, [pred_desc(dev, sv_rows, coef, held, bout, gamma, rho)])
        want = R.predict(x, sv_rows, coef, held, gamma, rho, out0)
        got = bout.get()
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert bad.size == 0, f"out differs at rows {bad[:8]}: device {got[bad[:8]]!r}, model {want[bad[:8]]!r}"
        if n_sv == 0:
            assert np.all(got[held] == -rho)
        assert np.array_equal(np.delete(got, held), np.delete(out0, held))
    return run


for _s in (0, 1, 15, 16, 17, 33):
    for _h in (1, 15, 16, 17, 40):
        CASES[f"predict-sv{_s}-held{_h}"] = predict_case(_s, _h)


@case("predict-two-problems")
def predict_two(dev):
    """two folds in one launch, 40 and 17 held-out rows, one target array"""
    m = 120
    rng = np.random.default_rng(6500)
    x = features(m, 6501)
    pick = rng.permutation(m)
    folds = [(pick[:40], np.sort(pick[40:73])), (pick[40:57], np.sort(pick[60:77]))]
    out0 = 1000.0 + np.arange(m)
    bx, bout = dev.buf(x), dev.buf(out0)
    descs, want = [], out0
    for held, sv_rows in folds:
        coef, rho = rng.uniform(-4.0, 4.0, len(sv_rows)), float(rng.uniform(-2, 2))
        descs.append(pred_desc(dev, sv_rows, coef, held, bout, 0.01, rho))
        want = R.predict(x, sv_rows, coef, held, 0.01, rho, want)
    launch_predict(dev, bx, descs)
    assert bout.get().tobytes() == want.tobytes()


@case("predict-exp-in-double")
def predict_exp(dev):
    """n_sv = 1, coef = 1, rho = 0, gamma = 1: out is the device's svt_exp_cr itself, a double, over 4,096 arguments spread over [-110, 0]"""
    m = 4096
    rng = np.random.default_rng(6600)
    x = features(m + 1, 6601)
    x[m] = 0.0                                                # the support vector
    target = rng.uniform(0.0, 110.0, m)
    x[:m] *= np.sqrt(target / (x[:m] * x[:m]).sum(axis=1))[:, None]
    held = rng.permutation(m)
    out0 = np.full(m + 1, -1.0)
    bx, bout = dev.buf(x), dev.buf(out0)
    launch_predict(dev, bx, [pred_desc(dev, [m], [1.0], held, bout, 1.0, 0.0)])
    want = R.predict(x, [m], [1.0], held, 1.0, 0.0, out0)
    got = bout.get()
    arg = -np.log(want[:m])
    assert arg.min() < 1.0 and arg.max() > 109.0 and np.all(want[:m] > 0)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size} of {m} values differ, first row {bad[0]}: device {got[bad[0]].hex()}, correctly rounded {want[bad[0]].hex()}"


@case("predict-exp-hard-arguments")
def predict_exp_hard(dev):
    """The same, at the 4,096 arguments of tests/golden/svt_exp_hard.txt, whose exp lies within 0.006 ulp of the midpoint of two doubles (of 400,000 in
    [-110, 0], tools/gen_svt_exp_hard.py): an exp good to an ulp rounds many of them the other way.  gamma is a problem's, not a row's, so this is one
    launch of 4,096 problems of one held-out row each: the row is the first unit vector, the support vector the zero row, |x - sv|^2 is 1 and the
    argument -gamma exactly."""
    args = np.array([float.fromhex(t) for t in open(os.path.join(ROOT, "tests", "golden", "svt_exp_hard.txt")).read().split()])
    m = len(args)
    assert m == 4096 and args.min() >= -110.0 and args.max() <= 0.0
    x = np.zeros((m + 1, R.NF))
    x[:m, 0] = 1.0
    out0 = np.full(m + 1, -1.0)
    bx, bout = dev.buf(x), dev.buf(out0)
    bs, bc, bh = dev.buf(np.array([m], dtype=np.int32)), dev.buf(np.array([1.0])), dev.buf(np.arange(m, dtype=np.int32))
    descs = [D.SvtPred(n_sv=1, n_held=1, sv_rows=bs.ptr, coef=bc.ptr, held=bh.ptr + 4 * k, out=bout.ptr, gamma=-float(v), rho=0.0) for k, v in enumerate(args)]
    launch_predict(dev, bx, descs)
    want = out0.copy()
    want[:m] = [(0.0 + 1.0 * R.exp_cr(v)) - 0.0 for v in args]
    for k in range(0, m, 512):                                # the model agrees with that shortcut
        assert R.predict(x, [m], [1.0], [k], -float(args[k]), 0.0, out0)[k] == want[k]
    got = bout.get()
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size} of {m} values differ, first argument {args[bad[0]].hex()}: device {got[bad[0]].hex()}, correctly rounded {want[bad[0]].hex()}"


# ---- the child: torch first, every case under its own time limit -----------------------------------------------------------------------------------
def worker(out_path):
    results = {}

    def save():
        with open(out_path + ".tmp", "w") as fh:
            json.dump(results, fh)
        os.replace(out_path + ".tmp", out_path)

    faulthandler.dump_traceback_later(CASE_LIMIT, exit=True)
    dev = D.Device()
    trouble = None
    for name in sorted(CASES):
        if trouble:
            results[name] = dict(ok=False, error="not run: " + trouble)
            continue
        faulthandler.dump_traceback_later(CASE_LIMIT, exit=True)
        t0 = time.time()
        try:
            CASES[name](dev)
            results[name] = dict(ok=True)
        except D.DeviceTrouble as e:
            trouble = f"{name} met trouble on the device: {e}"
            results[name] = dict(ok=False, error=trouble)
        except Exception:
            results[name] = dict(ok=False, error=traceback.format_exc()[-3000:])
        results[name]["seconds"] = round(time.time() - t0, 3)
        dev.release()
        save()
    faulthandler.cancel_dump_traceback_later()
    save()
    print(f"{sum(r['ok'] for r in results.values())} of {len(results)} cases ok in {sum(r.get('seconds', 0) for r in results.values()):.1f} s")


@pytest.fixture(autouse=True)
def _time_limit():
    """The child's device work runs under time limits of its own (CASE_LIMIT per case); this one ends a stuck parent with a traceback."""
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("svt") / "verdicts.json")
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_svt_kernels", out], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=800)
    res = json.load(open(out)) if os.path.exists(out) else {}
    return res, f"the child ended with status {p.returncode}: {p.stdout.decode()[-3000:]}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_against_its_model(verdicts, name):
    res, tail = verdicts
    assert name in res, f"{name} was not reached; {tail}"
    assert res[name]["ok"], res[name]["error"]


def test_the_child_ran_every_case_quickly(verdicts):
    res, tail = verdicts
    assert sorted(res) == sorted(CASES), tail
    slow = {k: v["seconds"] for k, v in res.items() if v.get("seconds", 0) > 5}
    assert not slow, f"cases over five seconds: {slow}"


if __name__ == "__main__":
    worker(sys.argv[1])
